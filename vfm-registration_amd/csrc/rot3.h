// rot3.h -- the rotation nearest to a 3x3 cross-covariance, in the fixed operation sequence that oracle/vfm_oracle.c restates
// (orc_rot_from_sigma).  One text for every kernel that needs it (ransac.hip: Kabsch; teaser.hip: the GNC-TLS rotation), so that their
// results agree bit for bit with the oracle and with each other.  fp64, compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int JACOBI_SWEEPS = 6;

// rotation from the 3x3 cross-covariance: one-sided Jacobi, fixed sweeps, only + - * / sqrt.
__device__ bool rot_from_sigma(const double S[9], double R[9]) {
    double G[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G[r][c] = S[r * 3 + c];
            V[r][c] = (r == c) ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int p = (e == 2) ? 1 : 0;
            const int q = (e == 0) ? 1 : 2;
            const double alpha = (G[0][p] * G[0][p] + G[1][p] * G[1][p]) + G[2][p] * G[2][p];
            const double beta = (G[0][q] * G[0][q] + G[1][q] * G[1][q]) + G[2][q] * G[2][q];
            const double gamma = (G[0][p] * G[0][q] + G[1][p] * G[1][q]) + G[2][p] * G[2][q];
            if (gamma == 0.0) continue;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double az = fabs(zeta);
            double tt = 1.0 / (az + sqrt(1.0 + zeta * zeta));
            if (zeta < 0.0) tt = -tt;
            const double c = 1.0 / sqrt(1.0 + tt * tt);
            const double s = c * tt;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double gp = G[r][p], gq = G[r][q];
                G[r][p] = c * gp - s * gq;
                G[r][q] = s * gp + c * gq;
                const double vp = V[r][p], vq = V[r][q];
                V[r][p] = c * vp - s * vq;
                V[r][q] = s * vp + c * vq;
            }
        }
    }
    double nn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nn[c] = (G[0][c] * G[0][c] + G[1][c] * G[1][c]) + G[2][c] * G[2][c];
    // two dominant columns, ties -> lowest column index (static indexing only: select by value)
    int i1 = 0;
    if (nn[1] > nn[i1 == 0 ? 0 : 1]) i1 = 1;
    {
        const double cur = (i1 == 0) ? nn[0] : nn[1];
        if (nn[2] > cur) i1 = 2;
    }
    int i2;
    {
        // candidates are the two columns != i1, scanned in ascending order, strict '>' to replace
        const int ca = (i1 == 0) ? 1 : 0;
        const int cb = (i1 == 2) ? 1 : 2;
        const double na = (ca == 0) ? nn[0] : nn[1];
        const double nb = (cb == 1) ? nn[1] : nn[2];
        i2 = (nb > na) ? cb : ca;
    }
    const double n1 = (i1 == 0) ? nn[0] : ((i1 == 1) ? nn[1] : nn[2]);
    const double n2 = (i2 == 0) ? nn[0] : ((i2 == 1) ? nn[1] : nn[2]);
    if (!(n1 > 0.0)) return false;
    if (!(n2 > n1 * 1e-20)) return false;
    const double s1 = sqrt(n1), s2 = sqrt(n2);
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double g1 = (i1 == 0) ? G[r][0] : ((i1 == 1) ? G[r][1] : G[r][2]);
        const double g2 = (i2 == 0) ? G[r][0] : ((i2 == 1) ? G[r][1] : G[r][2]);
        u1[r] = g1 / s1;
        u2[r] = g2 / s2;
        v1[r] = (i1 == 0) ? V[r][0] : ((i1 == 1) ? V[r][1] : V[r][2]);
        v2[r] = (i2 == 0) ? V[r][0] : ((i2 == 1) ? V[r][1] : V[r][2]);
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1];
    v3[1] = v1[2] * v2[0] - v1[0] * v2[2];
    v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c];
    return true;
}

}  // namespace
