// api_vocab.cpp -- part of the host side of libr3dm.so: pair proposal from bag-of-words view signatures (include/r3dm.h:
// r3dm_propose_pairs).  Vocabularies (an even sample of registered views gathered on the device, or the
// caller's rows), the signatures of views -- their rows quantised by the exhaustive matcher against the codebook staged as a private
// dataset view, counted by vocab_hist_kernel --, the all-pairs scores and the top-k selection.  The kernels are in kernels_vocab.hip;
// the sample is gathered by the head-gather kernels of kernels_match_head.hip.  There is no CPU fallback in this file: when HIP fails,
// the call fails.
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
    size_t row_bytes() const { return dtype == R3DM_F32 ? (size_t)dim * 4 : (size_t)dim; }
};

namespace {

void vocab_release(r3dm_vocab* v)
{
    (void)hipSetDevice(v->device);
    DevBuf* b[] = {&v->sig, &v->d_jobs, &v->d_list, &v->d_scores, &v->d_sel};
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
        R3DM_HIP(c, hipEventRecord(v->ev[0], c->stream));
        int rc = stage_into_slot(c, priv[0], 0, 0, 0, v->words.data(), v->n_words, v->dim, v->dtype, nullptr);
        if (rc != R3DM_OK) return rc;
        R3DM_HIP(c, hipEventRecord(v->ev[1], c->stream));
        R3DM_HIP(c, hipStreamSynchronize(c->stream));
        { float ms = 0.0f; if (hipEventElapsedTime(&ms, v->ev[0], v->ev[1]) == hipSuccess) v->report.ms_quantise += ms; }
        std::vector<int32_t> knn_idx;                          // (the matcher copies the first pair's lists back: room for them)
        std::vector<float> knn_dist;
        std::vector<VocabHistJob> hj;
        for (size_t b0 = 0; b0 < work.size();) {
            // a batch: at most 2^24 list slots (64 MiB of nn_idx, 128 MiB each of list indices and distances) and 32,768 views
            size_t b1 = b0;
            uint32_t max_n = 0;
            while (b1 < work.size()) {
                const uint32_t mn = std::max(max_n, work[b1].n);
                if (b1 > b0 && ((uint64_t)(b1 - b0 + 1) * match_q_stride(mn) > (1ull << 24) || b1 - b0 >= 32768)) break;
                max_n = mn; ++b1;
            }
            const uint32_t q_stride = match_q_stride(max_n);
            std::vector<PairJob> jobs;
            for (size_t k = b0; k < b1; ++k) jobs.push_back(PairJob{0u, c->imgs[work[k].slot]->view_id, priv[0], work[k].slot});
            knn_idx.resize((size_t)max_n * 2); knn_dist.resize((size_t)max_n * 2);
            R3DM_HIP(c, hipEventRecord(v->ev[0], c->stream));
            rc = run_match_batch(c, jobs, 1.0f, nullptr, knn_idx.data(), knn_dist.data());
            if (rc != R3DM_OK) return rc;
            R3DM_HIP(c, hipEventRecord(v->ev[1], c->stream));
            hj.clear();
            for (size_t k = b0; k < b1; ++k)
                hj.push_back(VocabHistJob{c->d_knn_idx.as<int32_t>() + (size_t)(k - b0) * q_stride * 2, work[k].n, v->sig.as<uint32_t>() + (size_t)work[k].row * v->stride});
            R3DM_HIP(c, v->d_jobs.ensure(hj.size() * sizeof(VocabHistJob)));
            R3DM_HIP(c, hipMemcpyAsync(v->d_jobs.p, hj.data(), hj.size() * sizeof(VocabHistJob), hipMemcpyHostToDevice, c->stream));
            R3DM_HIP(c, hipEventRecord(v->ev[2], c->stream));
            R3DM_HIP(c, launch_vocab_hist(c->stream, v->d_jobs.as<VocabHistJob>(), (uint32_t)hj.size(), max_n, v->n_words));
            R3DM_HIP(c, hipEventRecord(v->ev[3], c->stream));
            R3DM_HIP(c, hipStreamSynchronize(c->stream));      // the next batch overwrites the lists
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, v->ev[0], v->ev[1]) == hipSuccess) v->report.ms_quantise += ms;
            if (hipEventElapsedTime(&ms, v->ev[2], v->ev[3]) == hipSuccess) v->report.ms_histogram += ms;
            for (size_t k = b0; k < b1; ++k) v->report.n_rows_quantised += work[k].n;
            b0 = b1;
        }
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
    R3DM_HIP(c, hipMemsetAsync(v->d_scores.p, 0, score_bytes, c->stream));
    VocabScoreParams sp{};
    sp.sig = v->sig.as<uint32_t>(); sp.sig_row = v->d_list.as<uint32_t>(); sp.stride = v->stride; sp.n_views = V; sp.scores = v->d_scores.as<uint32_t>();
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

}  // namespace

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
