// hdbscan_host.cpp -- from the sorted spanning tree to HDBSCAN* labels on the host: single linkage, condensed tree, stabilities and
// excess-of-mass selection, as sklearn.cluster._hdbscan (_linkage.make_single_linkage, _tree._condense_tree, _compute_stability,
// _get_clusters, _do_labelling) computes them for allow_single_cluster=False, cluster_selection_epsilon=0, no max_cluster_size
// (hdbscan.HDBSCAN(min_cluster_size=100, min_samples=25).fit_predict of registration_node.py:735-736 reads the labels only).  Every
// floating-point sum is taken in the order that code takes it, so that tests/hdbscan_oracle.py can demand equal labels, not near ones.
// No HIP: sequential work on n - 1 edges.  This file includes nothing of the device side, so it also compiles alone for a host test
// program (tools/hdbscan_host_check.cpp).
#include <math.h>

#include <vector>

#include "../../include/vfmreg.h"

int vfm_fail(int code, const char* fmt, ...);

namespace {

struct Linkage {   // row i makes node n + i out of nodes left and right
    std::vector<int64_t> left, right, size;
    std::vector<double> lambda;
};

struct Condensed {   // rows (parent, child, lambda, size); a child below n is a point, the others are clusters numbered from n (the root)
    std::vector<int64_t> parent, child, size;
    std::vector<double> lambda;
    void add(int64_t p, int64_t c, double l, int64_t s) {
        parent.push_back(p);
        child.push_back(c);
        lambda.push_back(l);
        size.push_back(s);
    }
};

// breadth first from `root` over the linkage: out = root, its two nodes (left first), their nodes ...
void bfs(const Linkage& h, int64_t n, int64_t root, std::vector<int64_t>& out) {
    out.clear();
    out.push_back(root);
    for (size_t at = 0; at < out.size(); ++at) {
        const int64_t node = out[at];
        if (node >= n) {
            out.push_back(h.left[node - n]);
            out.push_back(h.right[node - n]);
        }
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int vfm_hdbscan_labels_host(const int32_t* lo, const int32_t* hi, const double* w2, int64_t n,
                                                                              int min_cluster_size, int32_t* labels_out) {
    if (n < 2 || n > ((int64_t)1 << 26)) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: n must be in 2..2^26");
    if (min_cluster_size < 2) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: min_cluster_size must be at least 2");
    if (!lo || !hi || !w2 || !labels_out) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: null pointer");
    const int64_t m = n - 1;
    for (int64_t e = 0; e < m; ++e) {
        if (!(lo[e] >= 0 && lo[e] < hi[e] && hi[e] < n)) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: edge %lld: 0 <= lo < hi < n does not hold", (long long)e);
        if (!(w2[e] >= 0.0)) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: edge %lld: w2 must be >= 0 and not a NaN", (long long)e);
        if (e > 0) {
            const bool after = w2[e - 1] < w2[e] || (w2[e - 1] == w2[e] && (lo[e - 1] < lo[e] || (lo[e - 1] == lo[e] && hi[e - 1] < hi[e])));
            if (!after) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: edge %lld: the edges must ascend strictly in (w2, lo, hi)", (long long)e);
        }
    }

    // single linkage: Kruskal over the tree's own edges in their order; a union-find whose roots carry their node
    Linkage h;
    h.left.resize(m), h.right.resize(m), h.size.resize(m), h.lambda.resize(m);
    {
        std::vector<int64_t> up(n), node(n), count(n, 1);
        for (int64_t i = 0; i < n; ++i) up[i] = node[i] = i;
        auto find = [&](int64_t x) {
            int64_t r = x;
            while (up[r] != r) r = up[r];
            while (up[x] != r) {
                const int64_t next = up[x];
                up[x] = r;
                x = next;
            }
            return r;
        };
        for (int64_t e = 0; e < m; ++e) {
            const int64_t a = find(lo[e]), b = find(hi[e]);
            if (a == b) return vfm_fail(VFM_EINVAL, "hdbscan_labels_host: edge %lld closes a cycle: not a spanning tree", (long long)e);
            h.left[e] = node[a];
            h.right[e] = node[b];
            h.size[e] = count[a] + count[b];
            h.lambda[e] = w2[e] > 0.0 ? 1.0 / sqrt(w2[e]) : INFINITY;
            const int64_t big = count[a] >= count[b] ? a : b, small = big == a ? b : a;
            up[small] = big;
            count[big] = h.size[e];
            node[big] = n + e;
        }
    }

    // condensed tree (_condense_tree)
    Condensed t;
    int64_t next_label = n + 1;
    {
        const int64_t root = 2 * m;
        std::vector<int64_t> relabel(root + 1, -1), nodes, sub;
        std::vector<unsigned char> ignore(root + 1, 0);
        relabel[root] = n;
        bfs(h, n, root, nodes);
        auto points_leave = [&](int64_t from, int64_t subtree, double lambda) {
            bfs(h, n, subtree, sub);
            for (const int64_t x : sub) {
                if (x < n) t.add(relabel[from], x, lambda, 1);
                ignore[x] = 1;
            }
        };
        for (const int64_t node : nodes) {
            if (ignore[node] || node < n) continue;
            const int64_t left = h.left[node - n], right = h.right[node - n];
            const double lambda = h.lambda[node - n];
            const int64_t left_count = left >= n ? h.size[left - n] : 1, right_count = right >= n ? h.size[right - n] : 1;
            const bool left_big = left_count >= min_cluster_size, right_big = right_count >= min_cluster_size;
            if (left_big && right_big) {
                relabel[left] = next_label++;
                t.add(relabel[node], relabel[left], lambda, left_count);
                relabel[right] = next_label++;
                t.add(relabel[node], relabel[right], lambda, right_count);
            } else if (!left_big && !right_big) {
                points_leave(node, left, lambda);
                points_leave(node, right, lambda);
            } else if (!left_big) {
                relabel[right] = relabel[node];
                points_leave(node, left, lambda);
            } else {
                relabel[left] = relabel[node];
                points_leave(node, right, lambda);
            }
        }
    }

    // stabilities (_compute_stability), clusters numbered c = label - n, 0 the root
    const int64_t clusters = next_label - n;
    const size_t rows = t.parent.size();
    std::vector<double> birth(clusters, NAN), stability(clusters, 0.0);
    std::vector<int64_t> up(clusters, 0);
    std::vector<std::vector<int64_t>> below(clusters);
    for (size_t r = 0; r < rows; ++r) {
        if (t.child[r] >= n) {
            birth[t.child[r] - n] = t.lambda[r];
            up[t.child[r] - n] = t.parent[r] - n;
            below[t.parent[r] - n].push_back(t.child[r] - n);
        }
    }
    birth[0] = 0.0;
    for (size_t r = 0; r < rows; ++r) {
        const int64_t p = t.parent[r] - n;
        stability[p] += (t.lambda[r] - birth[p]) * (double)t.size[r];
    }

    // excess of mass (_get_clusters): from the highest cluster down to the root's children; the root is never a cluster
    std::vector<unsigned char> chosen(clusters, 1);
    chosen[0] = 0;
    std::vector<int64_t> queue;
    for (int64_t c = clusters - 1; c >= 1; --c) {
        double subtree = 0.0;
        for (const int64_t d : below[c]) subtree += stability[d];
        if (subtree > stability[c]) {
            chosen[c] = 0;
            stability[c] = subtree;
        } else {
            queue.assign(below[c].begin(), below[c].end());
            for (size_t at = 0; at < queue.size(); ++at) {
                const int64_t d = queue[at];
                chosen[d] = 0;
                queue.insert(queue.end(), below[d].begin(), below[d].end());
            }
        }
    }

    // labels (_do_labelling): a point belongs to the chosen cluster it left, or that an unchosen cluster it left hangs under; a point
    // that reaches the root that way is noise.  Clusters are numbered in ascending label.
    std::vector<int64_t> top(clusters, 0), number(clusters, -1);   // top: the chosen cluster at or above c, 0 for none
    int64_t count = 0;
    for (int64_t c = 1; c < clusters; ++c) {
        top[c] = chosen[c] ? c : top[up[c]];
        if (chosen[c]) number[c] = count++;
    }
    for (size_t r = 0; r < rows; ++r) {
        if (t.child[r] >= n) continue;
        const int64_t c = top[t.parent[r] - n];
        labels_out[t.child[r]] = c == 0 ? -1 : (int32_t)number[c];
    }
    return VFM_OK;
}
