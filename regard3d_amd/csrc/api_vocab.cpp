// api_vocab.cpp -- part of the host side of libr3dm.so: pair proposal from bag-of-words view signatures (include/r3dm.h:
// r3dm_propose_pairs).  Vocabularies (an even sample of registered views gathered on the device, or the
// caller's rows), the signatures of views -- their rows quantised by the exhaustive matcher against the codebook staged as a private
// dataset view, counted by vocab_hist_kernel --, the all-pairs scores and the top-k selection.  The kernels are in kernels_vocab.hip;
// the sample is gathered by the head-gather kernels of kernels_match_head.hip.  Training (r3dm_vocab_train)
// iterates the same quantisation with Lloyd's update step between (kernels_vocab_train.hip, the stable sort of kernels_tracks.hip);
// idf weighting (r3dm_vocab_set_weighting) swaps the score kernel's instantiation and the selection's normaliser.  There is no CPU
// fallback in this file: when HIP fails, the call fails.
#include "r3dm_ctx.hpp"

struct r3dm_vocab {
    int device = 0;
    r3dm_dtype dtype = R3DM_F32;
    uint32_t dim = 0, n_words = 0;
    uint32_t stride = 0;                              // words between two signatures: n_words rounded up to a multiple of 4
    std::vector<unsigned char> words;                 // n_words rows of the vocabulary's type, as a caller would register them
    struct Sig { uint64_t serial; uint32_t n, row; }; // the registration it was counted from, its rows, its place in `sig`
    std::unordered_map<uint32_t, Sig> sigs;           // view id -> signature
    DevBuf sig;                                       // u32 [sig_cap][stride]
    uint32_t sig_cap = 0, sig_used = 0;
    DevBuf d_jobs, d_list, d_scores, d_sel;           // histogram jobs; (signature, rows, rank) of the listed views; scores; picks
    PinBuf pin;                                       // landing zone of the picks and the scores
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    r3dm_vocab_stats report{};
    int weighting = R3DM_VOCAB_WEIGHT_COUNTS;         // r3dm_vocab_set_weighting
    std::vector<uint32_t> q;                          // word weights of the last r3dm_propose_pairs call (all 1 under COUNTS)
    DevBuf d_q, d_df, d_W;                            // IDF: weights [stride], document frequencies [n_words], W [n_views] u64
    r3dm_vocab_train_stats train{};                   // r3dm_vocab_train_report
    size_t row_bytes() const { return dtype == R3DM_F32 ? (size_t)dim * 4 : (size_t)dim; }
};

namespace {

void vocab_release(r3dm_vocab* v)
{
    (void)hipSetDevice(v->device);
    DevBuf* b[] = {&v->sig, &v->d_jobs, &v->d_list, &v->d_scores, &v->d_sel, &v->d_q, &v->d_df, &v->d_W};
    for (DevBuf* x : b) x->release();
    v->pin.release();
    for (hipEvent_t& e : v->ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
}

struct VocabDeleter { void operator()(r3dm_vocab* v) const { if (v) { vocab_release(v); delete v; } } };
using VocabPtr = std::unique_ptr<r3dm_vocab, VocabDeleter>;

int vocab_args_ok(r3dm_ctx* c, uint32_t n_words, uint32_t dim, r3dm_dtype dtype)
{
    if (n_words < 2 || n_words > R3DM_VOCAB_MAX_WORDS) { c->err = "a vocabulary holds 2 .. 65,536 words"; return R3DM_ERR_INVALID; }
    if (dim == 0 || (dtype != R3DM_F32 && dtype != R3DM_U8 && dtype != R3DM_BIN)) return R3DM_ERR_INVALID;
    if (dtype == R3DM_BIN && !(((dim + 3) / 4) == 8 || ((dim + 3) / 4) == 16)) { c->err = "binary descriptors must be 29..32 or 61..64 bytes"; return R3DM_ERR_UNSUPPORTED; }
    return R3DM_OK;
}

VocabPtr vocab_new(r3dm_ctx* c, uint32_t n_words, uint32_t dim, r3dm_dtype dtype)
{
    VocabPtr v(new r3dm_vocab());
    v->device = c->device; v->dtype = dtype; v->dim = dim; v->n_words = n_words; v->stride = (n_words + 3u) / 4u * 4u;
    v->words.resize((size_t)n_words * v->row_bytes());
    v->q.assign(n_words, 1u);
    return v;
}

// the slots of the listed views: every id registered, listed once, and of type / length (dtype, dim) -- of the first view's when
// dim == 0 on entry, which then returns them
int listed_slots(r3dm_ctx* c, const uint32_t* ids, uint32_t n, r3dm_dtype& dtype, uint32_t& dim, std::vector<uint32_t>& slots)
{
    slots.resize(n);
    std::vector<uint32_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { c->err = "a view id is listed twice"; return R3DM_ERR_INVALID; }
    for (uint32_t k = 0; k < n; ++k) {
        auto it = c->slot_of.find(ids[k]);
        if (it == c->slot_of.end()) { c->err = "unregistered view"; return R3DM_ERR_INVALID; }
        const HostImage& h = *c->imgs[it->second];
        if (dim == 0) { dtype = h.dtype; dim = h.dim; }
        if (h.dtype != dtype || h.dim != dim) { c->err = "views of one type and one descriptor length only"; return R3DM_ERR_INVALID; }
        slots[k] = it->second;
    }
    return R3DM_OK;
}

int vocab_events(r3dm_ctx* c, r3dm_vocab* v)
{
    for (hipEvent_t& e : v->ev) if (!e) R3DM_HIP(c, hipEventCreate(&e));
    return R3DM_OK;
}

// room for `rows` signatures; the ones there are kept
int sig_reserve(r3dm_ctx* c, r3dm_vocab* v, uint32_t rows)
{
    if (rows <= v->sig_cap) return R3DM_OK;
    const uint32_t cap = std::max(rows, v->sig_cap * 2);
    DevBuf grown;
    R3DM_HIP(c, grown.ensure((size_t)cap * v->stride * 4));
    if (v->sig_used) {
        const hipError_t e = hipMemcpyAsync(grown.p, v->sig.p, (size_t)v->sig_used * v->stride * 4, hipMemcpyDeviceToDevice, c->stream);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
        if (e2 != hipSuccess) { grown.release(); c->err = std::string("signature copy: ") + hipGetErrorString(e2); return R3DM_ERR_HIP; }
    }
    v->sig.release();
    v->sig = grown; v->sig_cap = cap;
    return R3DM_OK;
}

// The quantisation both the signatures and the training run: the codebook staged into `priv_slot` as a dataset view, then the views of
// `work` as query sides through the exhaustive matcher, in batches of at most 2^24 list slots (64 MiB of nn_idx, 128 MiB each of list
// indices and distances) and 32,768 views, raw 2-lists kept on the device.  After each batch, `after(b0, b1, max_n, q_stride)` queues
// what reads the lists of work[b0 .. b1) -- view k's at d_knn_idx + (k - b0) * q_stride * 2 -- and the stream is synchronised before
// the next batch overwrites them.  The staging and every batch's matcher are timed on ev[0] / ev[1] into *ms_total; `after` has ev[2] /
// ev[3] for its own kernels.
struct QuantiseWork { uint32_t slot, n; };
template <class After>
int quantise_in_batches(r3dm_ctx* c, r3dm_vocab* v, uint32_t priv_slot, const std::vector<QuantiseWork>& work, double* ms_total, After&& after)
{
    R3DM_HIP(c, hipEventRecord(v->ev[0], c->stream));
    int rc = stage_into_slot(c, priv_slot, 0, 0, 0, v->words.data(), v->n_words, v->dim, v->dtype, nullptr);
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, hipEventRecord(v->ev[1], c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    { float ms = 0.0f; if (hipEventElapsedTime(&ms, v->ev[0], v->ev[1]) == hipSuccess) *ms_total += ms; }
    std::vector<int32_t> knn_idx;                              // (the matcher copies the first pair's lists back: room for them)
    std::vector<float> knn_dist;
    for (size_t b0 = 0; b0 < work.size();) {
        size_t b1 = b0;
        uint32_t max_n = 0;
        while (b1 < work.size()) {
            const uint32_t mn = std::max(max_n, work[b1].n);
            if (b1 > b0 && ((uint64_t)(b1 - b0 + 1) * match_q_stride(mn) > (1ull << 24) || b1 - b0 >= 32768)) break;
            max_n = mn; ++b1;
        }
        std::vector<PairJob> jobs;
        for (size_t k = b0; k < b1; ++k) jobs.push_back(PairJob{0u, c->imgs[work[k].slot]->view_id, priv_slot, work[k].slot});
        knn_idx.resize((size_t)max_n * 2); knn_dist.resize((size_t)max_n * 2);
        R3DM_HIP(c, hipEventRecord(v->ev[0], c->stream));
        rc = run_match_batch(c, jobs, 1.0f, nullptr, knn_idx.data(), knn_dist.data());
        if (rc != R3DM_OK) return rc;
        R3DM_HIP(c, hipEventRecord(v->ev[1], c->stream));
        rc = after(b0, b1, max_n, match_q_stride(max_n));
        if (rc != R3DM_OK) return rc;
        R3DM_HIP(c, hipStreamSynchronize(c->stream));          // the next batch overwrites the lists
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, v->ev[0], v->ev[1]) == hipSuccess) *ms_total += ms;
        b0 = b1;
    }
    return R3DM_OK;
}

// Every listed view holds a signature of its present registration afterwards; rows_out[k] = its place in v->sig.  The views to
// (re)build are quantised in batches of the exhaustive matcher -- codebook = dataset, view = queries, raw 2-lists kept on the device --
// and each batch's lists are counted where the matcher left them.
int ensure_signatures(r3dm_ctx* c, r3dm_vocab* v, const uint32_t* ids, const std::vector<uint32_t>& slots, std::vector<uint32_t>& rows_out)
{
    const uint32_t n = (uint32_t)slots.size();
    rows_out.resize(n);
    struct Todo { uint32_t slot, row, n; };
    std::vector<Todo> todo;
    uint32_t fresh = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const HostImage& h = *c->imgs[slots[k]];
        auto it = v->sigs.find(ids[k]);
        if (it != v->sigs.end() && it->second.serial == h.serial) { rows_out[k] = it->second.row; v->report.n_signatures_cached += 1; continue; }
        const uint32_t row = it != v->sigs.end() ? it->second.row : v->sig_used + fresh++;
        rows_out[k] = row;
        todo.push_back(Todo{slots[k], row, h.n});
    }
    if (todo.empty()) return R3DM_OK;
    { const int rc = sig_reserve(c, v, v->sig_used + fresh); if (rc != R3DM_OK) return rc; }
    v->sig_used += fresh;
    // a signature under construction is nobody's: the map learns of it when its histogram is queued
    for (const Todo& t : todo) v->sigs.erase(c->imgs[t.slot]->view_id);
    { const int rc = vocab_events(c, v); if (rc != R3DM_OK) return rc; }
    std::vector<Todo> work;
    for (const Todo& t : todo) {
        R3DM_HIP(c, hipMemsetAsync(v->sig.as<uint32_t>() + (size_t)t.row * v->stride, 0, (size_t)v->stride * 4, c->stream));
        if (t.n) work.push_back(t);
    }
    if (!work.empty()) {
        CallCounters counters(c, {});                          // r3dm_stats is left as the call found it
        PrivateSlots priv(c, 1);
        std::vector<QuantiseWork> qw;
        for (const Todo& t : work) qw.push_back(QuantiseWork{t.slot, t.n});
        std::vector<VocabHistJob> hj;
        const int rc = quantise_in_batches(c, v, priv[0], qw, &v->report.ms_quantise, [&](size_t b0, size_t b1, uint32_t max_n, uint32_t q_stride) -> int {
            hj.clear();
            for (size_t k = b0; k < b1; ++k)
                hj.push_back(VocabHistJob{c->d_knn_idx.as<int32_t>() + (size_t)(k - b0) * q_stride * 2, work[k].n, v->sig.as<uint32_t>() + (size_t)work[k].row * v->stride});
            R3DM_HIP(c, v->d_jobs.ensure(hj.size() * sizeof(VocabHistJob)));
            R3DM_HIP(c, hipMemcpyAsync(v->d_jobs.p, hj.data(), hj.size() * sizeof(VocabHistJob), hipMemcpyHostToDevice, c->stream));
            R3DM_HIP(c, hipEventRecord(v->ev[2], c->stream));
            R3DM_HIP(c, launch_vocab_hist(c->stream, v->d_jobs.as<VocabHistJob>(), (uint32_t)hj.size(), max_n, v->n_words));
            R3DM_HIP(c, hipEventRecord(v->ev[3], c->stream));
            R3DM_HIP(c, hipStreamSynchronize(c->stream));
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, v->ev[2], v->ev[3]) == hipSuccess) v->report.ms_histogram += ms;
            for (size_t k = b0; k < b1; ++k) v->report.n_rows_quantised += work[k].n;
            return R3DM_OK;
        });
        if (rc != R3DM_OK) return rc;
    }
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    for (const Todo& t : todo) {
        const HostImage& h = *c->imgs[t.slot];
        v->sigs[h.view_id] = r3dm_vocab::Sig{h.serial, h.n, t.row};
    }
    v->report.n_signatures_built += todo.size();
    return R3DM_OK;
}

int call_begin(r3dm_ctx* c, r3dm_vocab* v, const uint32_t* ids, uint32_t n_views, std::vector<uint32_t>& slots)
{
    if (!c || !v || !ids || n_views == 0) return R3DM_ERR_INVALID;
    if (v->device != c->device) { c->err = "the vocabulary belongs to another device"; return R3DM_ERR_INVALID; }
    r3dm_dtype dtype = v->dtype; uint32_t dim = v->dim;
    const int rc = listed_slots(c, ids, n_views, dtype, dim, slots);
    if (rc != R3DM_OK) return rc;
    R3DM_HIP(c, hipSetDevice(c->device));
    v->report = r3dm_vocab_stats{};
    return R3DM_OK;
}

int vocab_sample_impl(r3dm_ctx* c, const uint32_t* ids, uint32_t n_views, uint32_t n_words, r3dm_vocab** out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = nullptr;
    if (!ids || n_views == 0) return R3DM_ERR_INVALID;
    r3dm_dtype dtype = R3DM_F32; uint32_t dim = 0;
    std::vector<uint32_t> slots;
    int rc = listed_slots(c, ids, n_views, dtype, dim, slots);
    if (rc == R3DM_OK) rc = vocab_args_ok(c, n_words, dim, dtype);
    if (rc != R3DM_OK) return rc;
    uint64_t T = 0;
    for (uint32_t s : slots) T += c->imgs[s]->n;
    if (T < n_words) { c->err = "fewer rows in the listed views than words asked for"; return R3DM_ERR_INVALID; }
    R3DM_HIP(c, hipSetDevice(c->device));
    VocabPtr v = vocab_new(c, n_words, dim, dtype);
    // word t = row floor((2 t + 1) T / (2 n_words)) of the concatenation: both sides ascend, one walk deals the rows to their views
    const bool binary = dtype == R3DM_BIN;
    const HostImage& first = *c->imgs[slots[0]];
    const uint32_t per_row = binary ? first.words : first.G * 2;           // u32 / float4 per gathered row
    const size_t gathered_row = (size_t)per_row * (binary ? 4 : 16);
    std::vector<uint32_t> local(n_words), first_word(n_views + 1, 0);
    {
        uint64_t base = 0; uint32_t k = 0;
        for (uint32_t t = 0; t < n_words; ++t) {
            const uint64_t g = (2ull * t + 1ull) * T / (2ull * n_words);
            while (g >= base + c->imgs[slots[k]]->n) { base += c->imgs[slots[k]]->n; ++k; first_word[k] = t; }
            local[t] = (uint32_t)(g - base);
        }
        for (uint32_t j = k + 1; j <= n_views; ++j) first_word[j] = n_words;
    }
    DevBuf d_rows, d_out;
    struct Release { DevBuf &a, &b; ~Release() { a.release(); b.release(); } } release{d_rows, d_out};
    R3DM_HIP(c, d_rows.ensure((size_t)n_words * 4));
    R3DM_HIP(c, d_out.ensure((size_t)n_words * gathered_row));
    R3DM_HIP(c, hipMemcpyAsync(d_rows.p, local.data(), (size_t)n_words * 4, hipMemcpyHostToDevice, c->stream));
    for (uint32_t k = 0; k < n_views; ++k) {
        const uint32_t t0 = first_word[k], cnt = first_word[k + 1] - t0;
        if (!cnt) continue;
        const HostImage& h = *c->imgs[slots[k]];
        R3DM_HIP(c, launch_head_gather(c->stream, binary ? (const void*)h.bin.p : (const void*)h.tiled.p, d_rows.as<uint32_t>() + t0, cnt, per_row, binary,
                                       d_out.as<unsigned char>() + (size_t)t0 * gathered_row));
    }
    std::vector<unsigned char> back((size_t)n_words * gathered_row);
    R3DM_HIP(c, hipMemcpyAsync(back.data(), d_out.p, back.size(), hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    // gathered rows are padded (8 G floats, whole words): cut to the registered length, bytes back from the floats they became
    const size_t rb = v->row_bytes();
    for (uint32_t t = 0; t < n_words; ++t) {
        const unsigned char* src = back.data() + (size_t)t * gathered_row;
        unsigned char* dst = v->words.data() + (size_t)t * rb;
        if (dtype == R3DM_U8) { const float* f = reinterpret_cast<const float*>(src); for (uint32_t e = 0; e < dim; ++e) dst[e] = (unsigned char)f[e]; }
        else std::memcpy(dst, src, rb);
    }
    *out = v.release();
    return R3DM_OK;
}

int vocab_from_rows_impl(r3dm_ctx* c, const void* rows, uint32_t n_words, uint32_t dim, r3dm_dtype dtype, r3dm_vocab** out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = nullptr;
    if (!rows) return R3DM_ERR_INVALID;
    const int rc = vocab_args_ok(c, n_words, dim, dtype);
    if (rc != R3DM_OK) return rc;
    VocabPtr v = vocab_new(c, n_words, dim, dtype);
    std::memcpy(v->words.data(), rows, v->words.size());
    *out = v.release();
    return R3DM_OK;
}

int view_signatures_impl(r3dm_ctx* c, r3dm_vocab* v, const uint32_t* ids, uint32_t n_views, uint32_t* hist_out)
{
    std::vector<uint32_t> slots, rows;
    if (!hist_out) return R3DM_ERR_INVALID;
    int rc = call_begin(c, v, ids, n_views, slots);
    if (rc == R3DM_OK) rc = ensure_signatures(c, v, ids, slots, rows);
    if (rc != R3DM_OK) return rc;
    for (uint32_t k = 0; k < n_views; ++k)
        R3DM_HIP(c, hipMemcpyAsync(hist_out + (size_t)k * v->n_words, v->sig.as<uint32_t>() + (size_t)rows[k] * v->stride, (size_t)v->n_words * 4,
                                   hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    return R3DM_OK;
}

// 256 log2(N / df) as include/r3dm.h states it, N >= df >= 1: integers only, so the weight is the same on every host
uint32_t log2_q8(uint32_t N, uint32_t df)
{
    uint32_t e = 0;
    while (((uint64_t)df << (e + 1)) <= N) ++e;
    uint64_t x = (uint64_t)((((unsigned __int128)N) << (62 - e)) / df);        // Q1.62 in [2^62, 2^63)
    uint32_t q = e;
    for (int k = 0; k < 8; ++k) {
        x = (uint64_t)(((unsigned __int128)x * x) >> 62);
        q *= 2;
        if (x >= (1ull << 63)) { x >>= 1; q += 1; }
    }
    return q;
}

int propose_pairs_impl(r3dm_ctx* c, r3dm_vocab* v, const uint32_t* ids, uint32_t n_views, uint32_t top_k, uint32_t* pairs_out,
                       uint64_t cap_pairs, uint64_t* n_pairs_out, uint32_t* scores_out)
{
    if (!n_pairs_out) return R3DM_ERR_INVALID;
    *n_pairs_out = 0;
    if (top_k < 1) { if (c) c->err = "top_k >= 1"; return R3DM_ERR_INVALID; }
    if (cap_pairs < (uint64_t)n_views * top_k) { if (c) c->err = "pairs_out must hold n_views * top_k pairs"; return R3DM_ERR_INVALID; }
    if (!pairs_out || n_views > 65535u * kVocabTile) return R3DM_ERR_INVALID;
    std::vector<uint32_t> slots, rows;
    int rc = call_begin(c, v, ids, n_views, slots);
    if (rc == R3DM_OK) rc = ensure_signatures(c, v, ids, slots, rows);
    if (rc == R3DM_OK) rc = vocab_events(c, v);
    if (rc != R3DM_OK) return rc;
    const uint32_t V = n_views, kk = std::min(top_k, V - 1);
    // place of every listed view in view-id order, and back
    std::vector<uint32_t> order(V);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [ids](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
    std::vector<uint32_t> list(3 * (size_t)V);                 // signature | rows | rank
    for (uint32_t k = 0; k < V; ++k) { list[k] = rows[k]; list[V + k] = c->imgs[slots[k]]->n; list[2 * (size_t)V + order[k]] = k; }
    const size_t score_bytes = (size_t)V * V * 4, sel_bytes = (size_t)V * kk * 4;
    R3DM_HIP(c, v->d_list.ensure(list.size() * 4));
    R3DM_HIP(c, v->d_scores.ensure(score_bytes));
    R3DM_HIP(c, v->d_sel.ensure(std::max<size_t>(sel_bytes, 4)));
    R3DM_HIP(c, v->pin.ensure(sel_bytes + (scores_out ? score_bytes : 0) + 64));
    R3DM_HIP(c, hipMemcpyAsync(v->d_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, c->stream));
    v->q.assign(v->n_words, 1u);
    const bool idf = v->weighting == R3DM_VOCAB_WEIGHT_IDF;
    if (idf) {
        // the weights of this call's list, then the views' W in the place of their row counts
        uint32_t N = 0;
        for (uint32_t k = 0; k < V; ++k) N += c->imgs[slots[k]]->n != 0;
        R3DM_HIP(c, v->d_df.ensure((size_t)v->n_words * 4));
        R3DM_HIP(c, v->d_q.ensure((size_t)v->stride * 4));
        R3DM_HIP(c, v->d_W.ensure((size_t)V * 8));
        R3DM_HIP(c, launch_vocab_df(c->stream, v->sig.as<uint32_t>(), v->d_list.as<uint32_t>(), v->stride, V, v->n_words, v->d_df.as<uint32_t>()));
        std::vector<uint32_t> df(v->n_words), q(v->stride, 0u);
        R3DM_HIP(c, hipMemcpyAsync(df.data(), v->d_df.p, df.size() * 4, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t w = 0; w < v->n_words; ++w) q[w] = df[w] ? log2_q8(N, df[w]) : 0u;
        std::copy(q.begin(), q.begin() + v->n_words, v->q.begin());
        R3DM_HIP(c, hipMemcpyAsync(v->d_q.p, q.data(), q.size() * 4, hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, launch_vocab_weight_sums(c->stream, v->sig.as<uint32_t>(), v->d_list.as<uint32_t>(), v->stride, V, v->n_words, v->d_q.as<uint32_t>(),
                                             v->d_W.as<unsigned long long>()));
        std::vector<unsigned long long> W(V);
        R3DM_HIP(c, hipMemcpyAsync(W.data(), v->d_W.p, (size_t)V * 8, hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < V; ++k) {
            if (W[k] >= (1ull << 32)) { c->err = "idf-weighted signature sum W of a view reaches 2^32: fewer rows per view or COUNTS weighting"; return R3DM_ERR_UNSUPPORTED; }
            list[V + k] = (uint32_t)W[k];
        }
        R3DM_HIP(c, hipMemcpyAsync(v->d_list.as<uint32_t>() + V, list.data() + V, (size_t)V * 4, hipMemcpyHostToDevice, c->stream));
    }
    R3DM_HIP(c, hipMemsetAsync(v->d_scores.p, 0, score_bytes, c->stream));
    VocabScoreParams sp{};
    sp.sig = v->sig.as<uint32_t>(); sp.sig_row = v->d_list.as<uint32_t>(); sp.stride = v->stride; sp.n_views = V; sp.scores = v->d_scores.as<uint32_t>();
    sp.q = idf ? v->d_q.as<uint32_t>() : nullptr;
    {
        // slices of the word axis: enough workgroups for the chip when the tiles are few, at least 8 chunks each
        const uint32_t nt = (V + kVocabTile - 1) / kVocabTile, chunks = (v->stride + kVocabChunk - 1) / kVocabChunk;
        const uint64_t tiles = (uint64_t)nt * (nt + 1) / 2;
        uint32_t nz = (uint32_t)std::min<uint64_t>((512 + tiles - 1) / tiles, (chunks + 7) / 8);
        nz = std::max(nz, 1u);
        sp.words_per_z = (chunks + nz - 1) / nz * kVocabChunk;
        nz = (v->stride + sp.words_per_z - 1) / sp.words_per_z;
        R3DM_HIP(c, hipEventRecord(v->ev[0], c->stream));
        R3DM_HIP(c, launch_vocab_intersect(c->stream, sp, nz));
        R3DM_HIP(c, hipEventRecord(v->ev[1], c->stream));
    }
    VocabSelectParams lp{};
    lp.scores = sp.scores; lp.n_rows = v->d_list.as<uint32_t>() + V; lp.rank = v->d_list.as<uint32_t>() + 2 * (size_t)V; lp.n_views = V; lp.top_k = kk;
    lp.sel = v->d_sel.as<uint32_t>();
    R3DM_HIP(c, hipEventRecord(v->ev[2], c->stream));
    R3DM_HIP(c, launch_vocab_select(c->stream, lp));
    R3DM_HIP(c, hipEventRecord(v->ev[3], c->stream));
    uint32_t* sel = v->pin.as<uint32_t>();
    if (sel_bytes) R3DM_HIP(c, hipMemcpyAsync(sel, v->d_sel.p, sel_bytes, hipMemcpyDeviceToHost, c->stream));
    uint32_t* sc = reinterpret_cast<uint32_t*>(v->pin.as<unsigned char>() + (sel_bytes + 63) / 64 * 64);
    if (scores_out) R3DM_HIP(c, hipMemcpyAsync(sc, v->d_scores.p, score_bytes, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v->ev[0], v->ev[1]) == hipSuccess) v->report.ms_score = ms;
    if (hipEventElapsedTime(&ms, v->ev[2], v->ev[3]) == hipSuccess) v->report.ms_select = ms;
    if (scores_out) std::memcpy(scores_out, sc, score_bytes);
    // the union of the picks as (min id, max id), unique, by (I, J)
    std::vector<uint64_t> keys;
    keys.reserve((size_t)V * kk);
    for (uint32_t i = 0; i < V; ++i)
        for (uint32_t t = 0; t < kk; ++t) {
            const uint32_t r = sel[(size_t)i * kk + t];
            if (r == kNone) break;
            if (r >= V) { c->err = "selection kernel returned a rank out of range"; return R3DM_ERR_HIP; }
            const uint32_t a = ids[i], b = ids[order[r]];
            keys.push_back(((uint64_t)std::min(a, b) << 32) | std::max(a, b));
        }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    for (size_t p = 0; p < keys.size(); ++p) { pairs_out[2 * p] = (uint32_t)(keys[p] >> 32); pairs_out[2 * p + 1] = (uint32_t)keys[p]; }
    *n_pairs_out = keys.size();
    return R3DM_OK;
}

// the device buffers of one r3dm_vocab_train call: given back on every exit
struct TrainBufs {
    DevBuf assign, keys, vals, keys2, vals2, scratch, loc, base, views, counts, moved, jobs, blocks, first_block, sums, words;
    ~TrainBufs()
    {
        DevBuf* b[] = {&assign, &keys, &vals, &keys2, &vals2, &scratch, &loc, &base, &views, &counts, &moved, &jobs, &blocks, &first_block, &sums, &words};
        for (DevBuf* x : b) x->release();
    }
};

// One assignment of the training set against v's present words: assign[g] = word of row g, *moved = the rows whose entry changed,
// counts[w] = members of word w.  The batches are quantise_in_batches', as for the signatures; nothing depends on where they end.
int train_assign(r3dm_ctx* c, r3dm_vocab* v, const std::vector<uint32_t>& slots, const std::vector<uint32_t>& base, TrainBufs& B, uint32_t priv_slot,
                 uint32_t* moved, std::vector<uint32_t>& counts)
{
    std::vector<QuantiseWork> work;
    std::vector<uint32_t> g0;
    for (size_t k = 0; k < slots.size(); ++k)
        if (c->imgs[slots[k]]->n) { work.push_back(QuantiseWork{slots[k], c->imgs[slots[k]]->n}); g0.push_back(base[k]); }
    R3DM_HIP(c, hipMemsetAsync(B.moved.p, 0, 4, c->stream));
    R3DM_HIP(c, hipMemsetAsync(B.counts.p, 0, (size_t)v->n_words * 4, c->stream));
    std::vector<VocabAssignJob> aj;
    std::vector<VocabHistJob> hj;
    double ms_kernels = 0.0;
    const int rc = quantise_in_batches(c, v, priv_slot, work, &v->train.ms_assign, [&](size_t b0, size_t b1, uint32_t max_n, uint32_t q_stride) -> int {
        aj.clear(); hj.clear();
        for (size_t k = b0; k < b1; ++k) {
            const int32_t* idx = c->d_knn_idx.as<int32_t>() + (size_t)(k - b0) * q_stride * 2;
            aj.push_back(VocabAssignJob{idx, work[k].n, g0[k]});
            hj.push_back(VocabHistJob{idx, work[k].n, B.counts.as<uint32_t>()});
        }
        const size_t aj_bytes = (aj.size() * sizeof(VocabAssignJob) + 63) / 64 * 64;
        R3DM_HIP(c, B.jobs.ensure(aj_bytes + hj.size() * sizeof(VocabHistJob)));
        R3DM_HIP(c, hipMemcpyAsync(B.jobs.p, aj.data(), aj.size() * sizeof(VocabAssignJob), hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(B.jobs.as<unsigned char>() + aj_bytes, hj.data(), hj.size() * sizeof(VocabHistJob), hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipEventRecord(v->ev[2], c->stream));
        R3DM_HIP(c, launch_vocab_assign(c->stream, B.jobs.as<VocabAssignJob>(), (uint32_t)aj.size(), max_n, B.assign.as<uint32_t>(), B.moved.as<unsigned int>()));
        R3DM_HIP(c, launch_vocab_hist(c->stream, reinterpret_cast<const VocabHistJob*>(B.jobs.as<unsigned char>() + aj_bytes), (uint32_t)hj.size(), max_n, v->n_words));
        R3DM_HIP(c, hipEventRecord(v->ev[3], c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, v->ev[2], v->ev[3]) == hipSuccess) ms_kernels += ms;
        for (size_t k = b0; k < b1; ++k) v->train.n_rows_assigned += work[k].n;
        return R3DM_OK;
    });
    if (rc != R3DM_OK) return rc;
    v->train.ms_assign += ms_kernels;                          // the copy and count kernels belong to the assignment
    R3DM_HIP(c, hipMemcpyAsync(moved, B.moved.p, 4, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipMemcpyAsync(counts.data(), B.counts.p, (size_t)v->n_words * 4, hipMemcpyDeviceToHost, c->stream));
    R3DM_HIP(c, hipStreamSynchronize(c->stream));
    return R3DM_OK;
}

int vocab_train_impl(r3dm_ctx* c, const r3dm_vocab* init, const uint32_t* ids, uint32_t n_views, uint32_t max_iterations, r3dm_vocab** out)
{
    if (!c || !out) return R3DM_ERR_INVALID;
    *out = nullptr;
    if (!init || !ids || n_views == 0) return R3DM_ERR_INVALID;
    if (init->device != c->device) { c->err = "the vocabulary belongs to another device"; return R3DM_ERR_INVALID; }
    if (max_iterations == 0) { c->err = "max_iterations >= 1"; return R3DM_ERR_INVALID; }
    r3dm_dtype dtype = init->dtype; uint32_t dim = init->dim;
    std::vector<uint32_t> slots;
    int rc = listed_slots(c, ids, n_views, dtype, dim, slots);
    if (rc != R3DM_OK) return rc;
    std::vector<uint32_t> base(n_views + 1, 0);
    uint64_t T64 = 0;
    for (uint32_t k = 0; k < n_views; ++k) { base[k] = (uint32_t)T64; T64 += c->imgs[slots[k]]->n; }
    if (T64 == 0) { c->err = "no rows in the listed views"; return R3DM_ERR_INVALID; }
    if (T64 >= (1ull << 32)) { c->err = "a training set holds fewer than 2^32 rows"; return R3DM_ERR_UNSUPPORTED; }
    const uint32_t T = (uint32_t)T64;
    base[n_views] = T;
    R3DM_HIP(c, hipSetDevice(c->device));
    VocabPtr v = vocab_new(c, init->n_words, dim, dtype);
    v->words = init->words;
    rc = vocab_events(c, v.get());
    if (rc != R3DM_OK) return rc;
    const bool binary = dtype == R3DM_BIN;
    const uint32_t n_words = v->n_words;
    const HostImage* first = nullptr;
    for (uint32_t s : slots) if (c->imgs[s]->n) { first = c->imgs[s].get(); break; }
    VocabTrainParams P{};
    P.n_words = n_words; P.dim = dim;
    P.row_units = binary ? first->words : first->G * 2;
    P.pieces = binary ? first->words : (dim + 3) / 4;
    const size_t per_block = (size_t)P.pieces * (binary ? 32 * 4 : 4 * 8);          // bytes of a block's sums
    const uint64_t max_blocks = (uint64_t)T / kVocabTrainBlock + n_words;
    TrainBufs B;
    R3DM_HIP(c, B.assign.ensure((size_t)T * 4));
    for (DevBuf* x : {&B.keys, &B.vals, &B.keys2, &B.vals2}) R3DM_HIP(c, x->ensure((size_t)T * 4));
    R3DM_HIP(c, B.scratch.ensure(tracks_scratch_words(T, true) * 4));
    R3DM_HIP(c, B.loc.ensure((size_t)T * 8));
    R3DM_HIP(c, B.base.ensure((size_t)(n_views + 1) * 4));
    R3DM_HIP(c, B.views.ensure((size_t)n_views * sizeof(void*)));
    R3DM_HIP(c, B.counts.ensure((size_t)n_words * 4));
    R3DM_HIP(c, B.moved.ensure(4));
    R3DM_HIP(c, B.blocks.ensure((size_t)max_blocks * 8));
    R3DM_HIP(c, B.first_block.ensure((size_t)(n_words + 1) * 4));
    R3DM_HIP(c, B.sums.ensure((size_t)max_blocks * per_block));
    R3DM_HIP(c, B.words.ensure(v->words.size()));
    {
        std::vector<const void*> ptrs(n_views);
        for (uint32_t k = 0; k < n_views; ++k) ptrs[k] = binary ? c->imgs[slots[k]]->bin.p : c->imgs[slots[k]]->tiled.p;
        R3DM_HIP(c, hipMemcpyAsync(B.views.p, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(B.base.p, base.data(), base.size() * 4, hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipMemsetAsync(B.assign.p, 0xFF, (size_t)T * 4, c->stream));      // no word: every row moves at t = 0
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
    }
    P.views = B.views.as<const void*>(); P.loc = B.loc.as<uint2>(); P.blocks = B.blocks.as<uint2>(); P.first_block = B.first_block.as<uint32_t>();
    P.counts = B.counts.as<uint32_t>(); P.block_sums = B.sums.as<double>(); P.block_bits = B.sums.as<uint32_t>(); P.words = B.words.p;
    CallCounters counters(c, {});                              // r3dm_stats is left as the call found it
    PrivateSlots priv(c, 1);
    std::vector<uint32_t> counts(n_words), first_block(n_words + 1);
    std::vector<uint2> blocks;
    r3dm_vocab_train_stats& R = v->train;
    for (uint32_t t = 0;; ++t) {
        uint32_t moved = 0;
        rc = train_assign(c, v.get(), slots, base, B, priv[0], &moved, counts);
        if (rc != R3DM_OK) return rc;
        R.n_moved = t == 0 ? T : moved;
        R.n_empty = (uint64_t)std::count(counts.begin(), counts.end(), 0u);
        R.max_members = *std::max_element(counts.begin(), counts.end());
        if (t > 0 && moved == 0) { R.converged = 1; break; }
        // the members of every word in ascending g: a stable sort of g by a[g]
        R3DM_HIP(c, hipEventRecord(v->ev[0], c->stream));
        R3DM_HIP(c, launch_vocab_sort_keys(c->stream, B.assign.as<uint32_t>(), T, B.keys.as<uint32_t>(), B.vals.as<uint32_t>()));
        bool in_second = false;
        R3DM_HIP(c, tracks_sort_by_root(c->stream, B.scratch.as<uint32_t>(), B.keys.as<uint32_t>(), B.vals.as<uint32_t>(), B.keys2.as<uint32_t>(),
                                        B.vals2.as<uint32_t>(), T, 16, &in_second));
        R3DM_HIP(c, launch_vocab_locate(c->stream, (in_second ? B.vals2 : B.vals).as<uint32_t>(), T, B.base.as<uint32_t>(), n_views, B.loc.as<uint2>()));
        R3DM_HIP(c, hipEventRecord(v->ev[1], c->stream));
        // the tree: blocks of kVocabTrainBlock consecutive members of a word
        blocks.clear();
        uint32_t at = 0;
        for (uint32_t w = 0; w < n_words; ++w) {
            first_block[w] = (uint32_t)blocks.size();
            for (uint32_t m = 0; m < counts[w]; m += kVocabTrainBlock) blocks.push_back(make_uint2(at + m, std::min(kVocabTrainBlock, counts[w] - m)));
            at += counts[w];
        }
        first_block[n_words] = (uint32_t)blocks.size();
        if (at != T || blocks.size() > max_blocks) { c->err = "word counts do not add up to the training set"; return R3DM_ERR_HIP; }
        P.n_blocks = (uint32_t)blocks.size();
        R3DM_HIP(c, hipMemcpyAsync(B.blocks.p, blocks.data(), blocks.size() * 8, hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(B.first_block.p, first_block.data(), first_block.size() * 4, hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipMemcpyAsync(B.words.p, v->words.data(), v->words.size(), hipMemcpyHostToDevice, c->stream));
        R3DM_HIP(c, hipEventRecord(v->ev[2], c->stream));
        R3DM_HIP(c, launch_vocab_block_sums(c->stream, P, dtype));
        R3DM_HIP(c, launch_vocab_update(c->stream, P, dtype));
        R3DM_HIP(c, hipEventRecord(v->ev[3], c->stream));
        R3DM_HIP(c, hipMemcpyAsync(v->words.data(), B.words.p, v->words.size(), hipMemcpyDeviceToHost, c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, v->ev[0], v->ev[1]) == hipSuccess) R.ms_sort += ms;
        if (hipEventElapsedTime(&ms, v->ev[2], v->ev[3]) == hipSuccess) R.ms_update += ms;
        if (++R.n_updates == max_iterations) break;
    }
    *out = v.release();
    return R3DM_OK;
}

}  // namespace

extern "C" int r3dm_vocab_train(r3dm_ctx* c, const r3dm_vocab* init, const uint32_t* view_ids, uint32_t n_views, uint32_t max_iterations, r3dm_vocab** out)
{
    return r3dm_guarded(c, [&]() -> int { return vocab_train_impl(c, init, view_ids, n_views, max_iterations, out); });
}

extern "C" int r3dm_vocab_train_report(const r3dm_vocab* v, r3dm_vocab_train_stats* out)
{
    if (!v || !out) return R3DM_ERR_INVALID;
    *out = v->train;
    return R3DM_OK;
}

extern "C" int r3dm_vocab_set_weighting(r3dm_vocab* v, int mode)
{
    if (!v || (mode != R3DM_VOCAB_WEIGHT_COUNTS && mode != R3DM_VOCAB_WEIGHT_IDF)) return R3DM_ERR_INVALID;
    v->weighting = mode;
    return R3DM_OK;
}

extern "C" int r3dm_vocab_weights(const r3dm_vocab* v, uint32_t* q_out)
{
    if (!v || !q_out) return R3DM_ERR_INVALID;
    std::memcpy(q_out, v->q.data(), (size_t)v->n_words * 4);
    return R3DM_OK;
}

extern "C" int r3dm_vocab_sample(r3dm_ctx* c, const uint32_t* view_ids, uint32_t n_views, uint32_t n_words, r3dm_vocab** out)
{
    return r3dm_guarded(c, [&]() -> int { return vocab_sample_impl(c, view_ids, n_views, n_words, out); });
}

extern "C" int r3dm_vocab_from_rows(r3dm_ctx* c, const void* rows, uint32_t n_words, uint32_t dim, r3dm_dtype dtype, r3dm_vocab** out)
{
    return r3dm_guarded(c, [&]() -> int { return vocab_from_rows_impl(c, rows, n_words, dim, dtype, out); });
}

extern "C" int r3dm_vocab_info(const r3dm_vocab* v, uint32_t* n_words, uint32_t* dim, int32_t* dtype)
{
    if (!v) return R3DM_ERR_INVALID;
    if (n_words) *n_words = v->n_words;
    if (dim) *dim = v->dim;
    if (dtype) *dtype = (int32_t)v->dtype;
    return R3DM_OK;
}

extern "C" int r3dm_vocab_words(const r3dm_vocab* v, void* rows_out)
{
    if (!v || !rows_out) return R3DM_ERR_INVALID;
    std::memcpy(rows_out, v->words.data(), v->words.size());
    return R3DM_OK;
}

extern "C" void r3dm_vocab_free(r3dm_vocab* v)
{
    VocabDeleter()(v);
}

extern "C" int r3dm_view_signatures(r3dm_ctx* c, r3dm_vocab* v, const uint32_t* view_ids, uint32_t n_views, uint32_t* hist_out)
{
    return r3dm_guarded(c, [&]() -> int { return view_signatures_impl(c, v, view_ids, n_views, hist_out); });
}

extern "C" int r3dm_propose_pairs(r3dm_ctx* c, r3dm_vocab* v, const uint32_t* view_ids, uint32_t n_views, uint32_t top_k, uint32_t* pairs_out,
                                  uint64_t cap_pairs, uint64_t* n_pairs_out, uint32_t* scores_out)
{
    return r3dm_guarded(c, [&]() -> int { return propose_pairs_impl(c, v, view_ids, n_views, top_k, pairs_out, cap_pairs, n_pairs_out, scores_out); });
}

extern "C" int r3dm_vocab_report(const r3dm_vocab* v, r3dm_vocab_stats* out)
{
    if (!v || !out) return R3DM_ERR_INVALID;
    *out = v->report;
    return R3DM_OK;
}
