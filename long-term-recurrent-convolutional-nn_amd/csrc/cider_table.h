// cider_table.h -- the host side of CIDEr-D over token ids (include/lrcn_cider.h): the tables cider.hip uploads, built once from the
// references.  Plain C++ with no HIP in it, so that it compiles and is checked on a CPU alone (tests/test_cider_table_host.py); the one
// function the kernel shares, cider_hash, carries the device qualifier only under hipcc.
//
// Per n = 1..4:
//   keys [slots][n] int32, idf [slots] double   open addressing with linear probing over the distinct n-grams of all references; slots is a
//                                               power of two and at least twice their number, so a probe sequence always meets an empty
//                                               slot.  An empty slot has keys[slot][0] = -1 (ids are >= 0).  A look-up compares all n ids.
//   ent_off [n_refs + 1], ent [..] (slot, count) the distinct n-grams of reference r, ascending by slot
//   rnorm [n_refs]                              |v_r| = sqrt(sum (count * idf)^2), summed in the order the n-grams first occur in the reference
//                                               (cider.py's dict order), one term after the other
// idf = log(N) - log(max(1, df)) in double, df = the number of images one of whose references holds the n-gram: cider.py's form.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define LRCN_CIDER_HD __host__ __device__
#else
#define LRCN_CIDER_HD
#endif

namespace lrcn_cider_host {

constexpr int NMAX = 4;

// where the probe sequence of an n-gram starts (before the mask).  Only a starting point: equality is always decided on the full key.
LRCN_CIDER_HD inline uint32_t cider_hash(const int32_t *w, int n) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < n; ++k) {
        h ^= (uint64_t)(uint32_t)w[k];
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    return (uint32_t)(h ^ (h >> 29));
}

struct Entry {
    int32_t slot, count;
};

struct Tables {
    int n_images = 0, n_refs = 0, V = 0;
    double log_n = 0.0;
    int64_t ngrams[NMAX] = {0, 0, 0, 0};
    uint32_t slots[NMAX] = {0, 0, 0, 0};
    std::vector<int32_t> keys[NMAX];
    std::vector<double> idf[NMAX];
    std::vector<int32_t> ent_off[NMAX];
    std::vector<Entry> ent[NMAX];
    std::vector<double> rnorm[NMAX];
    std::vector<int32_t> ref_len;   // [n_refs]
    std::vector<int32_t> img_off;   // [n_images + 1]
    std::vector<int32_t> img_ref;   // [n_refs]: image i's references, in the order given, are img_ref[img_off[i] .. img_off[i+1])
};

// the slot holding `w`, or the empty slot its probe sequence ends in
inline uint32_t probe(const std::vector<int32_t> &keys, uint32_t mask, const int32_t *w, int n) {
    uint32_t s = cider_hash(w, n) & mask;
    for (;;) {
        const int32_t *k = &keys[(size_t)s * n];
        if (k[0] < 0) return s;
        bool eq = true;
        for (int j = 0; j < n; ++j) eq = eq && k[j] == w[j];
        if (eq) return s;
        s = (s + 1) & mask;
    }
}

inline uint32_t pow2_at_least(uint64_t x) {
    uint64_t p = 2;
    while (p < x) p <<= 1;
    return (uint32_t)p;
}

// Validates the arguments of lrcn_cider_create and fills `t`.  Returns "" or the message of the LRCN_EINVAL.
inline std::string build_tables(int n_images, int n_refs, const int32_t *ref_image, const int64_t *ref_offsets, const int32_t *ref_tokens, int V,
                                Tables &t) {
    if (!ref_image || !ref_offsets || !ref_tokens) return "null reference array";
    if (n_images < 1) return "n_images=" + std::to_string(n_images) + " must be >= 1";
    if (n_refs < 0) return "n_refs=" + std::to_string(n_refs) + " must be >= 0";
    if (V < 1) return "V=" + std::to_string(V) + " must be >= 1";
    if (ref_offsets[0] != 0) return "ref_offsets[0] must be 0";
    for (int r = 0; r < n_refs; ++r) {
        if (ref_offsets[r + 1] < ref_offsets[r]) return "ref_offsets decrease at reference " + std::to_string(r);
        if (ref_image[r] < 0 || ref_image[r] >= n_images)
            return "ref_image[" + std::to_string(r) + "]=" + std::to_string(ref_image[r]) + " outside [0," + std::to_string(n_images) + ")";
    }
    const int64_t total = ref_offsets[n_refs];
    if (total >= (1ll << 29)) return "2^29 or more reference words";
    for (int64_t k = 0; k < total; ++k)
        if (ref_tokens[k] < 0 || ref_tokens[k] >= V)
            return "reference word " + std::to_string(k) + " is " + std::to_string(ref_tokens[k]) + ", outside [0," + std::to_string(V) + ")";

    t = Tables();
    t.n_images = n_images;
    t.n_refs = n_refs;
    t.V = V;
    t.log_n = std::log((double)n_images);
    t.ref_len.resize(n_refs);
    for (int r = 0; r < n_refs; ++r) t.ref_len[r] = (int32_t)(ref_offsets[r + 1] - ref_offsets[r]);
    // references by image, in the order given (a counting sort)
    t.img_off.assign(n_images + 1, 0);
    for (int r = 0; r < n_refs; ++r) t.img_off[ref_image[r] + 1]++;
    for (int i = 0; i < n_images; ++i) t.img_off[i + 1] += t.img_off[i];
    t.img_ref.resize(n_refs);
    {
        std::vector<int32_t> at(t.img_off.begin(), t.img_off.end() - 1);
        for (int r = 0; r < n_refs; ++r) t.img_ref[at[ref_image[r]]++] = r;
    }

    for (int n = 1; n <= NMAX; ++n) {
        const int q = n - 1;
        int64_t positions = 0;
        for (int r = 0; r < n_refs; ++r) positions += std::max(0, t.ref_len[r] - n + 1);
        // first pass: a table large enough for every position, to count the distinct n-grams and the images that hold each
        uint32_t cap = pow2_at_least(2 * (uint64_t)std::max<int64_t>(1, positions));
        std::vector<int32_t> keys((size_t)cap * n, -1);
        std::vector<int32_t> df(cap, 0), last(cap, -1);
        int64_t distinct = 0;
        for (int i = 0; i < n_images; ++i)
            for (int k = t.img_off[i]; k < t.img_off[i + 1]; ++k) {
                const int r = t.img_ref[k];
                const int32_t *w = ref_tokens + ref_offsets[r];
                for (int p = 0; p + n <= t.ref_len[r]; ++p) {
                    const uint32_t s = probe(keys, cap - 1, w + p, n);
                    if (keys[(size_t)s * n] < 0) {
                        std::copy(w + p, w + p + n, &keys[(size_t)s * n]);
                        ++distinct;
                    }
                    if (last[s] != i) {
                        last[s] = i;
                        ++df[s];
                    }
                }
            }
        // the table that is uploaded: at least twice the distinct count, filled in the first table's slot order
        const uint32_t slots = pow2_at_least(2 * (uint64_t)std::max<int64_t>(1, distinct));
        t.ngrams[q] = distinct;
        t.slots[q] = slots;
        t.keys[q].assign((size_t)slots * n, -1);
        t.idf[q].assign(slots, 0.0);
        for (uint32_t s0 = 0; s0 < cap; ++s0) {
            if (keys[(size_t)s0 * n] < 0) continue;
            const uint32_t s = probe(t.keys[q], slots - 1, &keys[(size_t)s0 * n], n);
            std::copy(&keys[(size_t)s0 * n], &keys[(size_t)s0 * n] + n, &t.keys[q][(size_t)s * n]);
            t.idf[q][s] = t.log_n - std::log((double)std::max(1, df[s0]));
        }
        // per reference: (slot, count) of its distinct n-grams, and |v_r|
        t.ent_off[q].assign(n_refs + 1, 0);
        t.ent[q].clear();
        t.rnorm[q].assign(n_refs, 0.0);
        std::vector<std::pair<int32_t, int32_t>> sp;   // (slot, position)
        struct First {
            int32_t pos, slot, count;
        };
        std::vector<First> firsts;
        for (int r = 0; r < n_refs; ++r) {
            const int32_t *w = ref_tokens + ref_offsets[r];
            sp.clear();
            firsts.clear();
            for (int p = 0; p + n <= t.ref_len[r]; ++p) sp.emplace_back((int32_t)probe(t.keys[q], slots - 1, w + p, n), p);
            std::sort(sp.begin(), sp.end());
            for (size_t a = 0; a < sp.size();) {
                size_t b = a;
                while (b < sp.size() && sp[b].first == sp[a].first) ++b;
                firsts.push_back({sp[a].second, sp[a].first, (int32_t)(b - a)});
                t.ent[q].push_back({sp[a].first, (int32_t)(b - a)});
                a = b;
            }
            t.ent_off[q][r + 1] = (int32_t)t.ent[q].size();
            std::sort(firsts.begin(), firsts.end(), [](const First &x, const First &y) { return x.pos < y.pos; });
            double sum = 0.0;
            for (const First &f : firsts) {
                const double x = f.count * t.idf[q][f.slot];
                sum += x * x;
            }
            t.rnorm[q][r] = std::sqrt(sum);
        }
    }
    return "";
}

}  // namespace lrcn_cider_host
