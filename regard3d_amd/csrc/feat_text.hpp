// feat_text.hpp -- the reader of a .feat file (host only, no HIP: the facade includes it, and a host test compiles it alone).
#pragma once

#include <charconv>
#include <cstdio>
#include <string>
#include <system_error>
#include <vector>

namespace r3dm_feat {

// .feat: one "x y scale orientation" text line per feature; .desc: 8-byte count + raw rows
// (/root/reference/src/keypointSet.hpp:49-67 -> OpenMVG loadFeatsFromFile / loadDescsFromBinFile)
// scale: when given, receives the third column as written, one per feature (the priority of preemptive matching)
inline bool load_feat(const std::string& path, std::vector<float>& xy, std::vector<float>* scale = nullptr)
{
    // the whole file in one buffer, one from_chars per field (what `stream >> float` does, without the stream): groups of four
    // numbers until the first group that is not complete, like `while (f >> x >> y >> s >> o)`
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<char> txt;
    bool ok = fseek(f, 0, SEEK_END) == 0;
    const long sz = ok ? ftell(f) : -1;
    ok = ok && sz >= 0 && fseek(f, 0, SEEK_SET) == 0;
    if (ok) { txt.resize((size_t)sz + 1); ok = fread(txt.data(), 1, (size_t)sz, f) == (size_t)sz; txt[(size_t)sz] = 0; }
    fclose(f);
    if (!ok) return false;
    xy.clear();
    if (scale) scale->clear();
    // locale-independent, like the classic-locale `stream >> float` of OpenMVG's reader (the host application calls
    // setlocale(LC_ALL, ""), so strtof would read "12.5" as 12 under a comma-decimal locale): std::from_chars, after the white
    // space and the optional sign that operator>> accepts; hex / inf / nan tokens are not numbers for operator>> and end the file here too
    const char* s = txt.data();
    const char* const end_txt = s + (size_t)sz;
    for (;;) {
        float v[4];
        int k = 0;
        for (; k < 4; ++k) {
            while (s < end_txt && (*s == ' ' || *s == '\n' || *s == '\t' || *s == '\r' || *s == '\f' || *s == '\v')) ++s;
            const char* t = s;
            bool neg = false;
            if (t < end_txt && (*t == '+' || *t == '-')) { neg = *t == '-'; ++t; }
            if (t >= end_txt || !((*t >= '0' && *t <= '9') || *t == '.')) break;
            const std::from_chars_result r = std::from_chars(t, end_txt, v[k], std::chars_format::general);
            if (r.ec == std::errc::invalid_argument) break;
            if (r.ec == std::errc::result_out_of_range) v[k] = 0.0f;     // (never for pixel coordinates) operator>> sets failbit; keep going with 0
            if (neg) v[k] = -v[k];
            s = r.ptr;
        }
        if (k < 4) break;
        xy.push_back(v[0]); xy.push_back(v[1]);
        if (scale) scale->push_back(v[2]);
    }
    return true;
}

}  // namespace r3dm_feat
