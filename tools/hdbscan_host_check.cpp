// hdbscan_host_check.cpp -- a stand-alone host program around vfm_hdbscan_labels_host (csrc/hdbscan_host.cpp) for sanitizer runs: a
// few hand-made spanning trees whose labels are known, and the refusals.  No HIP, no GPU:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/hdbscan_host_check.cpp vfm-registration_amd/csrc/hdbscan_host.cpp -o /tmp/hdbscan_host_check && /tmp/hdbscan_host_check
// Exit status 0 and "ok" when every tree gives its labels.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../include/vfmreg.h"

static char g_err[512];
int vfm_fail(int code, const char* fmt, ...) {   // (error.cpp's, which is part of the HIP library)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct Tree {
    std::vector<int32_t> lo, hi;
    std::vector<double> w2;
    void add(int a, int b, double w) {
        lo.push_back(std::min(a, b));
        hi.push_back(std::max(a, b));
        w2.push_back(w);
    }
    void sort() {
        std::vector<size_t> at(lo.size());
        std::iota(at.begin(), at.end(), 0);
        std::sort(at.begin(), at.end(), [&](size_t a, size_t b) {
            if (w2[a] != w2[b]) return w2[a] < w2[b];
            if (lo[a] != lo[b]) return lo[a] < lo[b];
            return hi[a] < hi[b];
        });
        Tree t;
        for (size_t k : at) t.add(lo[k], hi[k], w2[k]);
        *this = t;
    }
    int64_t n() const { return (int64_t)lo.size() + 1; }
};

static int failures = 0;

static std::vector<int32_t> labels_of(Tree t, int min_cluster_size, int expect_rc = VFM_OK) {
    t.sort();
    std::vector<int32_t> labels(t.n(), -7);
    const int rc = vfm_hdbscan_labels_host(t.lo.data(), t.hi.data(), t.w2.data(), t.n(), min_cluster_size, labels.data());
    if (rc != expect_rc) {
        printf("FAIL: rc %d, expected %d (%s)\n", rc, expect_rc, g_err);
        ++failures;
    }
    return labels;
}

static void expect(const char* name, const std::vector<int32_t>& got, const std::vector<int32_t>& want) {
    if (got != want) {
        printf("FAIL: %s:", name);
        for (int32_t l : got) printf(" %d", l);
        printf("\n");
        ++failures;
    }
}

// `sides` paths of `count` points with light edges, joined in a chain by heavy ones
static Tree paths(int sides, int count, double light, double heavy) {
    Tree t;
    for (int s = 0; s < sides; ++s) {
        for (int k = 1; k < count; ++k) t.add(s * count + k - 1, s * count + k, light + 0.001 * k);
        if (s) t.add(s * count - 1, s * count, heavy * s);
    }
    return t;
}

int main() {
    {   // two sides of exactly min_cluster_size points: two clusters, the lower node first
        std::vector<int32_t> want(10, 0);
        std::fill(want.begin() + 5, want.end(), 1);
        const std::vector<int32_t> got = labels_of(paths(2, 5, 1.0, 50.0), 5);
        // which side is the left node is decided by the heavy edge's lower endpoint (point 4): its side is cluster 0
        expect("two sides of exactly min_cluster_size", got, want);
    }
    expect("one fewer than min_cluster_size per side", labels_of(paths(2, 4, 1.0, 50.0), 5), std::vector<int32_t>(8, -1));
    {   // three sides: the root splits into (0..9 | 10..14) at the heaviest edge, then 0..9 into two
        const std::vector<int32_t> got = labels_of(paths(3, 5, 1.0, 50.0), 5);
        bool ok = true;
        for (int s = 0; s < 3; ++s)
            for (int k = 0; k < 5; ++k) ok = ok && got[s * 5 + k] == got[s * 5] && got[s * 5] >= 0;
        ok = ok && got[0] != got[5] && got[5] != got[10] && got[0] != got[10];
        if (!ok) expect("three sides", got, {});
    }
    {   // all weights equal, a star: no split has two sides of min_cluster_size
        Tree t;
        for (int k = 1; k < 30; ++k) t.add(0, k, 2.0);
        expect("star", labels_of(t, 5), std::vector<int32_t>(30, -1));
    }
    {   // w2 == 0 inside both sides: lambda = +inf, stabilities +inf
        Tree t = paths(2, 6, 0.0, 3.0);
        for (double& w : t.w2) w = w < 1.0 ? 0.0 : w;
        Tree zero_sorted;   // equal weights must still ascend in (lo, hi)
        for (size_t k = 0; k < t.lo.size(); ++k) zero_sorted.add(t.lo[k], t.hi[k], t.w2[k]);
        std::vector<int32_t> want(12, 0);
        std::fill(want.begin() + 6, want.end(), 1);
        expect("w2 == 0", labels_of(zero_sorted, 6), want);
    }
    {   // a long path: the breadth-first orders are as deep as the tree
        Tree t;
        for (int k = 1; k < 20000; ++k) t.add(k - 1, k, (k % 5000 == 0) ? 1000.0 : 1.0 + (k % 7) * 0.01);
        const std::vector<int32_t> got = labels_of(t, 100);
        if (!(got[0] >= 0 && got[0] == got[4999] && got[5000] != got[0] && got[19999] >= 0)) expect("long path", {got[0], got[4999], got[5000], got[19999]}, {});
    }
    expect("two points", labels_of(paths(1, 2, 1.0, 0.0), 2), std::vector<int32_t>(2, -1));
    {   // refusals
        Tree t = paths(2, 4, 1.0, 50.0);
        (void)labels_of(t, 1, VFM_EINVAL);
        Tree cycle = t;
        cycle.lo[0] = cycle.lo[1], cycle.hi[0] = cycle.hi[1], cycle.w2[0] = cycle.w2[1] + 0.0001;
        (void)labels_of(cycle, 5, VFM_EINVAL);
        Tree nan = t;
        nan.w2[2] = NAN;
        std::vector<int32_t> labels(nan.n());
        if (vfm_hdbscan_labels_host(nan.lo.data(), nan.hi.data(), nan.w2.data(), nan.n(), 5, labels.data()) != VFM_EINVAL) ++failures;
        if (vfm_hdbscan_labels_host(nullptr, nan.hi.data(), nan.w2.data(), nan.n(), 5, labels.data()) != VFM_EINVAL) ++failures;
        if (vfm_hdbscan_labels_host(t.lo.data(), t.hi.data(), t.w2.data(), 1, 5, labels.data()) != VFM_EINVAL) ++failures;
    }
    printf(failures ? "%d failure(s)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
