// teaser_host.cpp -- the two sequential stages of TEASER++ registration (registration_node.py:91-159) on the host:
//   vfm_teaser_max_clique_host       PMC_EXACT's answer on the graph the device's reduction left (teaser.hip): THE maximum clique, the one
//                                    whose ascending index list is lexicographically smallest
//   vfm_teaser_tls_translation_host  TEASER's scalar TLS estimator per axis: a sweep over 2k sorted interval endpoints
// A search whose input is what the device left, and recurrences of at most 2k steps: neither has work for a GPU.  No HIP: this file
// includes nothing of the device side, so it also compiles alone for a host test program (tools/teaser_host_check.cpp).
// tests/teaser_oracle.py restates both.
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/vfmreg.h"

int vfm_fail(int code, const char* fmt, ...);

namespace {

typedef uint64_t Word;

struct CliqueSearch {
    const Word* adj;       // k rows of W words
    int64_t k, W;
    int64_t best;          // the size to beat: a clique is recorded when it is LARGER
    int64_t nodes, node_limit;
    bool exhausted;
    std::vector<int32_t> current, record;
    std::vector<std::vector<Word>> level;   // the candidate set of each depth
    std::vector<Word> uncoloured, cls;

    const Word* row(int64_t v) const { return adj + v * W; }

    static int64_t count(const std::vector<Word>& s) {
        int64_t c = 0;
        for (const Word w : s) c += __builtin_popcountll(w);
        return c;
    }

    // the number of colours of a greedy colouring of the graph on P: classes are filled one after the other, each by ascending index.
    // A clique takes a colour per member, so no clique inside P is larger.
    int64_t colours(const std::vector<Word>& P, int64_t stop_at) {
        uncoloured = P;
        int64_t used = 0;
        for (;;) {
            bool any = false;
            cls = uncoloured;
            for (int64_t w = 0; w < W; ++w) {
                while (cls[w]) {
                    any = true;
                    const int b = __builtin_ctzll(cls[w]);
                    const int64_t v = w * 64 + b;
                    uncoloured[w] &= ~((Word)1 << b);
                    cls[w] &= ~((Word)1 << b);
                    const Word* a = row(v);
                    for (int64_t q = w; q < W; ++q) cls[q] &= ~a[q];
                }
            }
            if (!any) return used;
            if (++used >= stop_at) return used;   // (enough to know that the branch is not pruned)
        }
    }

    // `current` is a clique of `size` members; level[size] holds the vertices above its last member that are adjacent to all of them
    void expand(int64_t size) {
        if (exhausted) return;
        if (++nodes > node_limit) {
            exhausted = true;
            return;
        }
        if (size > best) {
            best = size;
            record = current;
        }
        std::vector<Word>& P = level[size];
        int64_t left = count(P);
        if (left == 0 || size + left <= best) return;
        if (size + colours(P, best - size + 1) <= best) return;
        if ((int64_t)level.size() <= size + 1) level.emplace_back(W);
        for (int64_t w = 0; w < W; ++w) {
            while (P[w]) {
                if (size + left <= best) return;   // (what is left cannot beat the record even if it were one clique)
                const int b = __builtin_ctzll(P[w]);
                const int64_t v = w * 64 + b;
                P[w] &= ~((Word)1 << b);
                --left;
                std::vector<Word>& next = level[size + 1];
                const Word* a = row(v);
                for (int64_t q = 0; q < w; ++q) next[q] = 0;
                for (int64_t q = w; q < W; ++q) next[q] = P[q] & a[q];   // (P holds indices above v only)
                current.push_back((int32_t)v);
                expand(size + 1);
                current.pop_back();
                if (exhausted) return;
            }
        }
    }
};

}  // namespace

extern "C" __attribute__((visibility("default"))) int vfm_teaser_max_clique_host(const uint64_t* sub, const int32_t* kept, int64_t k,
                                                                                 int64_t known, int64_t node_limit, int32_t* clique_out,
                                                                                 int64_t* size_out) {
    if (k < 0 || k > 32768) return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: k must be in 0..32768");
    if (known < 0 || known > k) return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: known must be in 0..k (the size of a clique that exists)");
    if (node_limit < 1) return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: node_limit must be at least 1");
    if (!size_out || (k > 0 && (!sub || !kept || !clique_out))) return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: null pointer");
    const int64_t W = (k + 63) / 64;
    for (int64_t v = 0; v < k; ++v) {
        if (kept[v] < 0 || (v > 0 && kept[v] <= kept[v - 1]))
            return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: kept[%lld]: the original indices must ascend strictly from 0 or above", (long long)v);
        const Word* a = sub + v * W;
        if ((a[v >> 6] >> (v & 63)) & 1) return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: row %lld: the diagonal must be clear", (long long)v);
        if ((k & 63) && (a[W - 1] >> (k & 63))) return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: row %lld: the padding bits must be clear", (long long)v);
    }
    if (k == 0) {
        *size_out = 0;
        return VFM_OK;
    }
    // a graph that is itself one clique (what the reduction leaves when the heuristic found the maximum clique and nothing ties with it)
    bool complete = true;
    for (int64_t v = 0; v < k && complete; ++v) {
        int64_t d = 0;
        for (int64_t q = 0; q < W; ++q) d += __builtin_popcountll(sub[v * W + q]);
        complete = d == k - 1;
    }
    if (complete) {
        for (int64_t v = 0; v < k; ++v) clique_out[v] = kept[v];
        *size_out = k;
        return VFM_OK;
    }
    CliqueSearch s{};
    s.adj = sub;
    s.k = k;
    s.W = W;
    s.best = known > 0 ? known - 1 : 0;
    s.nodes = 0;
    s.node_limit = node_limit;
    s.exhausted = false;
    s.uncoloured.resize(W);
    s.cls.resize(W);
    s.level.reserve((size_t)k + 2);   // (a level per depth; never reallocated: expand() holds references into it)
    s.level.emplace_back(W);
    for (int64_t v = 0; v < k; ++v) s.level[0][v >> 6] |= (Word)1 << (v & 63);
    s.expand(0);
    if (s.exhausted)
        return vfm_fail(VFM_ELIMIT, "teaser_max_clique_host: the search visited node_limit = %lld nodes without finishing: no clique is returned",
                        (long long)node_limit);
    if (s.record.empty())   // (symmetric rows are not checked: only a `known` above the clique number, or such rows, lead here)
        return vfm_fail(VFM_EINVAL, "teaser_max_clique_host: no clique of known = %lld members exists", (long long)known);
    for (size_t i = 0; i < s.record.size(); ++i) clique_out[i] = kept[s.record[i]];
    *size_out = (int64_t)s.record.size();
    return VFM_OK;
}

extern "C" __attribute__((visibility("default"))) int vfm_teaser_tls_translation_host(const double* v, int64_t k, double range, double* t_out,
                                                                                      uint8_t* inliers_out) {
    if (k < 1 || k > 32768) return vfm_fail(VFM_EINVAL, "teaser_tls_translation_host: k must be in 1..32768");
    if (!(range > 0.0) || !(range < INFINITY)) return vfm_fail(VFM_EINVAL, "teaser_tls_translation_host: range must be positive and finite");
    if (!v || !t_out || !inliers_out) return vfm_fail(VFM_EINVAL, "teaser_tls_translation_host: null pointer");
    for (int64_t i = 0; i < 3 * k; ++i)
        if (!(fabs(v[i]) < INFINITY)) return vfm_fail(VFM_EINVAL, "teaser_tls_translation_host: v[%lld] is not finite", (long long)i);
    const double w = 1.0 / (range * range);
    std::vector<std::pair<double, int64_t>> h(2 * k);
    for (int a = 0; a < 3; ++a) {
        for (int64_t i = 0; i < k; ++i) {
            h[2 * i] = std::make_pair(v[3 * i + a] - range, i + 1);
            h[2 * i + 1] = std::make_pair(v[3 * i + a] + range, -(i + 1));
        }
        std::sort(h.begin(), h.end());   // (pairs: the value, then the signed index; no two entries are equal)
        int64_t card = 0;
        double dot_w = 0.0, dot_vw = 0.0, sum_v = 0.0, sum_sq = 0.0, outside = 0.0;
        for (int64_t i = 0; i < k; ++i) outside = outside + range;
        double best_cost = INFINITY, best_x = 0.0;
        bool have = false;
        for (int64_t e = 0; e < 2 * k; ++e) {
            const int64_t i = (h[e].second > 0 ? h[e].second : -h[e].second) - 1;
            const double eps = h[e].second > 0 ? 1.0 : -1.0;
            const double x = v[3 * i + a];
            card += h[e].second > 0 ? 1 : -1;
            dot_w = dot_w + eps * w;
            dot_vw = dot_vw + (eps * w) * x;
            outside = outside - eps * range;
            sum_v = sum_v + eps * x;
            sum_sq = sum_sq + (eps * x) * x;
            if (card == 0) continue;   // an empty consensus set has no estimate
            const double x_hat = dot_vw / dot_w;
            const double cost = (((double)card * (x_hat * x_hat) + sum_sq) - (2.0 * sum_v) * x_hat) + outside;
            if (!have || cost < best_cost) {
                have = true;
                best_cost = cost;
                best_x = x_hat;
            }
        }
        t_out[a] = best_x;
    }
    for (int64_t i = 0; i < k; ++i) {
        bool in = true;
        for (int a = 0; a < 3; ++a) in = in && fabs(v[3 * i + a] - t_out[a]) <= range;
        inliers_out[i] = in ? 1 : 0;
    }
    return VFM_OK;
}
