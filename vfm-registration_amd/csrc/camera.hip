// camera.hip -- the RobotCar camera front end: oxford_robotcar.py:103-136 of the reference.
//   vfm_demosaic_bilinear   colour_demosaicing.demosaicing_CFA_Bayer_bilinear: uint8 mosaic -> float32 RGB on 0..255
//   vfm_undistort_lut       robotcar_sdk CameraModel.undistort: scipy's map_coordinates(order=1) per channel, fp64, unfused
//   vfm_rectify_bayer       demosaic -> undistort -> astype(uint8) -> crop -> PIL resize(BILINEAR) for a whole rig: every output
//                           pixel demosaics the 4 x 4 mosaic window under its four taps on the fly; the demosaiced image is never
//                           written and cropped rows are never computed
// All three are gathers bounded by the 16-byte table entry per pixel: the table is read once, one double2 per lane, and the
// mosaic bytes come from cache.  The file is built with -ffp-contract=off: the fp64 chains below are the reference's, unfused.
#include <string.h>

#include "common.h"

namespace {

// colour (0 R, 1 G, 2 B) of mosaic position (y & 1, x & 1), two bits each, position y * 2 + x from bit 0
__host__ __device__ inline unsigned bayer_code(int pattern) {
    switch (pattern) {
        case VFM_BAYER_RGGB: return 0u | 1u << 2 | 1u << 4 | 2u << 6;
        case VFM_BAYER_GBRG: return 1u | 2u << 2 | 0u << 4 | 1u << 6;
        case VFM_BAYER_GRBG: return 1u | 0u << 2 | 2u << 4 | 1u << 6;
        default:             return 2u | 1u << 2 | 1u << 4 | 0u << 6;   // VFM_BAYER_BGGR
    }
}

// scipy.ndimage's `reflect` border (d c b a | a b c d) for i in [-1, n + 1], n >= 2
__device__ inline int reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// The N x N mosaic window whose top-left pixel is (r, c), border reflected: value | colour << 8 per pixel.  The mask moves with the
// reflected pixel (the library convolves the MASKED mosaic), so a pixel mirrored across the border keeps its own colour.
template <int N>
struct BayerWindow {
    int px[N][N];
    __device__ BayerWindow(const uint8_t* __restrict__ m, int H, int W, unsigned code, int r, int c) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int y = reflect(r + i, H);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int x = reflect(c + j, W);
                px[i][j] = (int)m[(int64_t)y * W + x] | (int)((code >> (2 * ((y & 1) * 2 + (x & 1)))) & 3u) << 8;
            }
        }
    }
    // 4 x (R, G, B) of the pixel at window position (a + 1, b + 1): sums of uint8 values with the weights of
    // [[1,2,1],[2,4,2],[1,2,1]] (R, B) and [[0,1,0],[1,4,1],[0,1,0]] (G); the division by 4 is exact in any float format
    __device__ void rgb4(int a, int b, int s[3]) const {
        s[0] = s[1] = s[2] = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int p = px[a + dy][b + dx], v = p & 255, col = p >> 8;
                const int w_rb = (dy == 1 ? 2 : 1) * (dx == 1 ? 2 : 1);
                const int w_g = (dy == 1 && dx == 1) ? 4 : ((dy == 1 || dx == 1) ? 1 : 0);
                s[0] += col == 0 ? v * w_rb : 0;
                s[1] += col == 1 ? v * w_g : 0;
                s[2] += col == 2 ? v * w_rb : 0;
            }
    }
};

// map_coordinates(order=1, mode='constant') at (row y, column x) of an H x W image: inside iff 0 <= y <= H-1 and 0 <= x <= W-1
// (false for NaN and infinities), first tap (r0, c0), weights w0 = 1 - f and w1 = 1 - w0 (not f: that differs in the last bit)
struct LutSample {
    bool inside;
    int r0, c0;
    double wr[2], wc[2];
};
__device__ inline LutSample lut_sample(double x, double y, int H, int W) {
    LutSample s;
    s.inside = y >= 0.0 && y <= (double)(H - 1) && x >= 0.0 && x <= (double)(W - 1);
    const double fy = floor(s.inside ? y : 0.0), fx = floor(s.inside ? x : 0.0);
    s.r0 = (int)fy;
    s.c0 = (int)fx;
    s.wr[0] = 1.0 - ((s.inside ? y : 0.0) - fy);
    s.wr[1] = 1.0 - s.wr[0];
    s.wc[0] = 1.0 - ((s.inside ? x : 0.0) - fx);
    s.wc[1] = 1.0 - s.wc[0];
    return s;
}
// t = 0, then t = t + (v[a][b] * wr[a]) * wc[b] in the order (0,0), (0,1), (1,0), (1,1)
__device__ inline double lut_blend(const LutSample& s, double v00, double v01, double v10, double v11) {
    double t = 0.0;
    t = t + (v00 * s.wr[0]) * s.wc[0];
    t = t + (v01 * s.wr[0]) * s.wc[1];
    t = t + (v10 * s.wr[1]) * s.wc[0];
    t = t + (v11 * s.wr[1]) * s.wc[1];
    return t;
}

__device__ inline uint8_t to_out(double t, uint8_t) {   // scipy's integer output: t + 0.5 truncated, clamped
    const int v = (int)(t + 0.5);
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
__device__ inline float to_out(double t, float) { return (float)t; }
__device__ inline double to_out(double t, double) { return t; }

// A workgroup's 256 consecutive RGB pixels, first pixel p0 of `total`, to out[3 * p0 ...]: staged in LDS and written as dwords
// where `out` is 4-byte aligned (3 * 256 bytes per workgroup keep that alignment), bytes otherwise and at the tail.
__device__ inline void store_rgb_block(uint8_t* __restrict__ out, int64_t p0, int64_t total, uint8_t r, uint8_t g, uint8_t b) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[768];
    const int t = threadIdx.x;
    stage[3 * t] = r;
    stage[3 * t + 1] = g;
    stage[3 * t + 2] = b;
    __syncthreads();
    const int64_t left = total - p0;
    const int nbytes = 3 * (int)(left < 256 ? left : 256);
    uint8_t* dst = out + 3 * p0;
    if ((reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
        if (4 * t + 4 <= nbytes) reinterpret_cast<uint32_t*>(dst)[t] = reinterpret_cast<const uint32_t*>(stage)[t];
        else
            for (int k = 4 * t; k < nbytes && k < 4 * t + 4; ++k) dst[k] = stage[k];
    } else {
        for (int k = t; k < nbytes; k += 256) dst[k] = stage[k];
    }
}

__global__ __launch_bounds__(256) void demosaic_bilinear_kernel(const uint8_t* __restrict__ cfa, int H, int W, unsigned code,
                                                                float* __restrict__ rgb) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
    const BayerWindow<3> win(cfa, H, W, code, r - 1, c - 1);
    int s[3];
    win.rgb4(0, 0, s);
    rgb[3 * p] = (float)s[0] * 0.25f;
    rgb[3 * p + 1] = (float)s[1] * 0.25f;
    rgb[3 * p + 2] = (float)s[2] * 0.25f;
}

template <typename T>
__global__ __launch_bounds__(256) void undistort_lut_kernel(const T* __restrict__ img, int H, int W, int C, const double2* __restrict__ lut,
                                                            T* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const double2 xy = lut[p];
    const LutSample s = lut_sample(xy.x, xy.y, H, W);
    // a tap past the last row / column has weight exactly 0 and reads the clamped pixel
    const int r1 = min(s.r0 + 1, H - 1), c1 = min(s.c0 + 1, W - 1);
    const T* a = img + ((int64_t)s.r0 * W + s.c0) * C;
    const T* b = img + ((int64_t)s.r0 * W + c1) * C;
    const T* c = img + ((int64_t)r1 * W + s.c0) * C;
    const T* d = img + ((int64_t)r1 * W + c1) * C;
    for (int ch = 0; ch < C; ++ch) {
        const double t = s.inside ? lut_blend(s, (double)a[ch], (double)b[ch], (double)c[ch], (double)d[ch]) : 0.0;
        out[p * C + ch] = to_out(t, T());
    }
}

struct RectifyCam {
    const uint8_t* mosaic;
    const double2* table;
    uint8_t* full;      // the cropped full-resolution image: the output (subsample 1) or a workspace region (subsample 2)
    uint8_t* half;      // subsample 2: the output
    int H, W, Hc;       // Hc = H - crop_bottom
    unsigned code;
    unsigned block0;    // first workgroup of this camera in the launch it takes part in
};
struct RectifyArgs {
    RectifyCam cam[VFM_RECTIFY_MAX_CAMS];
    int ncam;
};

// the camera workgroup `block` belongs to (block0 ascends; wave-uniform)
__device__ inline int camera_of(const RectifyArgs& a, unsigned block) {
    int k = 0;
    for (int i = 1; i < a.ncam; ++i) k = block >= a.cam[i].block0 ? i : k;
    return k;
}

// One thread per pixel of the cropped rectified image, 256 consecutive pixels per workgroup (the table rows and the output bytes
// of a cropped image are both contiguous).  numpy's astype(uint8) of the non-negative fp64 value: truncate, keep the low 8 bits
// (573.75 at a saturated red corner of the outermost ring becomes 61).  A sample outside the frame is exactly (0, 0, 0).
__global__ __launch_bounds__(256) void rectify_bayer_kernel(RectifyArgs a) {
    const RectifyCam& cam = a.cam[camera_of(a, blockIdx.x)];
    const int64_t total = (int64_t)cam.Hc * cam.W;
    const int64_t p0 = (int64_t)(blockIdx.x - cam.block0) * 256, p = p0 + threadIdx.x;
    uint8_t rgb[3] = {0, 0, 0};
    if (p < total) {
        const double2 xy = cam.table[p];
        const LutSample s = lut_sample(xy.x, xy.y, cam.H, cam.W);
        if (s.inside) {
            // taps (r0 + a, c0 + b): their 3 x 3 neighbourhoods are the 4 x 4 window from (r0 - 1, c0 - 1).  Where r0 = H - 1 the
            // second row of taps lies past the frame with weight exactly 0: the reflected window keeps its value finite.
            const BayerWindow<4> win(cam.mosaic, cam.H, cam.W, cam.code, s.r0 - 1, s.c0 - 1);
            int v[2][2][3];
            win.rgb4(0, 0, v[0][0]);
            win.rgb4(0, 1, v[0][1]);
            win.rgb4(1, 0, v[1][0]);
            win.rgb4(1, 1, v[1][1]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double t = lut_blend(s, v[0][0][ch] * 0.25, v[0][1][ch] * 0.25, v[1][0][ch] * 0.25, v[1][1][ch] * 0.25);
                rgb[ch] = (uint8_t)((int)t & 255);
            }
        }
    }
    store_rgb_block(cam.full, p0, total, rgb[0], rgb[1], rgb[2]);
}

// Pillow's 8-bit bilinear resampling by the factor 2 (ImagingResample: precompute_coeffs, normalize_coeffs_8bpc): output index i
// of n_in / 2 reads taps 2i-1 .. 2i+2 clipped to the image with triangle weights 1, 3, 3, 1 over their sum S (8 inside, 7 at the
// two ends, 6 for a 2-pixel line), each rounded to 22 fractional bits: k = floor(w / S * 2^22 + 0.5) = (w * 2^23 + S) / (2 S).
constexpr int PIL_BITS = 32 - 8 - 2;
struct PilTaps {
    int lo, n;
    int k[4];
};
__device__ inline PilTaps pil_taps(int i, int n_in) {
    PilTaps t;
    t.lo = max(2 * i - 1, 0);
    t.n = min(2 * i + 3, n_in) - t.lo;
    int w[4], S = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = t.lo + j;
        w[j] = j < t.n ? ((x == 2 * i - 1 || x == 2 * i + 2) ? 1 : 3) : 0;
        S += w[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) t.k[j] = (int)(((int64_t)w[j] << (PIL_BITS + 1)) + S) / (2 * S);
    return t;
}
__device__ inline int pil_clip8(int acc) {
    const int v = acc >> PIL_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// PIL's resize((W / 2, Hc / 2), BILINEAR) of the cropped image: the horizontal pass of the (up to) four source rows, rounded to
// uint8 as Pillow's intermediate image is, then the vertical pass.  One thread per output pixel.
__global__ __launch_bounds__(256) void resize2_bilinear_kernel(RectifyArgs a) {
    const RectifyCam& cam = a.cam[camera_of(a, blockIdx.x)];
    const int Wo = cam.W / 2, Ho = cam.Hc / 2;
    const int64_t total = (int64_t)Ho * Wo;
    const int64_t p0 = (int64_t)(blockIdx.x - cam.block0) * 256, p = p0 + threadIdx.x;
    uint8_t rgb[3] = {0, 0, 0};
    if (p < total) {
        const int yo = (int)(p / Wo), xo = (int)(p - (int64_t)yo * Wo);
        const PilTaps tx = pil_taps(xo, cam.W), ty = pil_taps(yo, cam.Hc);
        int acc[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
        for (int i = 0; i < ty.n; ++i) {
            const uint8_t* row = cam.full + ((int64_t)(ty.lo + i) * cam.W + tx.lo) * 3;
            int h[3] = {1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1), 1 << (PIL_BITS - 1)};
            for (int j = 0; j < tx.n; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) h[ch] += (int)row[3 * j + ch] * tx.k[j];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch] += pil_clip8(h[ch]) * ty.k[i];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = (uint8_t)pil_clip8(acc[ch]);
    }
    store_rgb_block(cam.half, p0, total, rgb[0], rgb[1], rgb[2]);
}

constexpr int64_t MAX_SIDE = 32768;   // 3 * H * W and every workgroup count stay far inside their integer types

inline bool pattern_ok(int pattern) { return pattern >= VFM_BAYER_RGGB && pattern <= VFM_BAYER_BGGR; }
inline unsigned blocks_of(int64_t pixels) { return (unsigned)((pixels + 255) / 256); }

// argument checks shared by the workspace query and the call; *ws_bytes = what the subsample-2 cameras need
int rectify_check(int ncam, const vfm_rectify_camera* cams, size_t* ws_bytes) {
    VFM_CHECK_ARG(cams && ncam >= 1 && ncam <= VFM_RECTIFY_MAX_CAMS, "rectify: 1..%d cameras per call (got %d)", VFM_RECTIFY_MAX_CAMS, ncam);
    VfmCarver carve(nullptr);
    for (int c = 0; c < ncam; ++c) {
        const vfm_rectify_camera& h = cams[c];
        VFM_CHECK_ARG(h.H >= 2 && h.W >= 2 && h.H <= MAX_SIDE && h.W <= MAX_SIDE, "rectify: camera %d: frame %lld x %lld (2..%lld a side)", c,
                      (long long)h.H, (long long)h.W, (long long)MAX_SIDE);
        VFM_CHECK_ARG(pattern_ok(h.pattern), "rectify: camera %d: unknown Bayer pattern %d", c, h.pattern);
        VFM_CHECK_ARG(h.crop_bottom >= 0 && h.crop_bottom < h.H, "rectify: camera %d: crop_bottom %lld of %lld rows", c,
                      (long long)h.crop_bottom, (long long)h.H);
        VFM_CHECK_ARG(h.subsample == 1 || h.subsample == 2, "rectify: camera %d: subsample %d (1 or 2)", c, h.subsample);
        const int64_t Hc = h.H - h.crop_bottom;
        VFM_CHECK_ARG(h.subsample == 1 || (Hc % 2 == 0 && h.W % 2 == 0),
                      "rectify: camera %d: cropped size %lld x %lld is not divisible by the subsample factor 2", c, (long long)Hc, (long long)h.W);
        if (h.subsample == 2) carve.take<uint8_t>((size_t)(3 * Hc * h.W));
    }
    *ws_bytes = carve.used();
    return VFM_OK;
}

}  // namespace

VFM_EXPORT int vfm_demosaic_bilinear(const uint8_t* cfa, int64_t H, int64_t W, int pattern, float* rgb_out, vfm_stream_t stream) {
    VFM_CHECK_ARG(cfa && rgb_out, "demosaic: null pointer");
    VFM_CHECK_ARG(H >= 2 && W >= 2 && H <= MAX_SIDE && W <= MAX_SIDE, "demosaic: frame %lld x %lld (2..%lld a side)", (long long)H, (long long)W,
                  (long long)MAX_SIDE);
    VFM_CHECK_ARG(pattern_ok(pattern), "demosaic: unknown Bayer pattern %d", pattern);
    hipLaunchKernelGGL(demosaic_bilinear_kernel, dim3(blocks_of(H * W)), dim3(256), 0, (hipStream_t)stream, cfa, (int)H, (int)W,
                       bayer_code(pattern), rgb_out);
    VFM_CHECK_LAUNCH("demosaic_bilinear_kernel");
    return VFM_OK;
}

VFM_EXPORT int vfm_undistort_lut(const void* image, int dtype, int64_t H, int64_t W, int C, const double* lut, void* out,
                                 vfm_stream_t stream) {
    VFM_CHECK_ARG(image && lut && out, "undistort: null pointer");
    VFM_CHECK_ARG(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE && C >= 1 && C <= 64, "undistort: image %lld x %lld x %d", (long long)H,
                  (long long)W, C);
    VFM_CHECK_ARG((reinterpret_cast<uintptr_t>(lut) & 15u) == 0, "undistort: the look-up table must be 16-byte aligned");
    const dim3 grid(blocks_of(H * W)), block(256);
    const double2* t = reinterpret_cast<const double2*>(lut);
    switch (dtype) {
        case VFM_IMAGE_U8:
            hipLaunchKernelGGL(undistort_lut_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)image, (int)H, (int)W, C, t,
                               (uint8_t*)out);
            break;
        case VFM_IMAGE_F32:
            hipLaunchKernelGGL(undistort_lut_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)image, (int)H, (int)W, C, t,
                               (float*)out);
            break;
        case VFM_IMAGE_F64:
            hipLaunchKernelGGL(undistort_lut_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)image, (int)H, (int)W, C, t,
                               (double*)out);
            break;
        default:
            return vfm_fail(VFM_EINVAL, "undistort: unknown image dtype %d", dtype);
    }
    VFM_CHECK_LAUNCH("undistort_lut_kernel");
    return VFM_OK;
}

VFM_EXPORT size_t vfm_rectify_bayer_workspace_bytes(int ncam, const vfm_rectify_camera* cams_host) {
    size_t bytes = 0;
    return rectify_check(ncam, cams_host, &bytes) == VFM_OK ? bytes : 0;
}

VFM_EXPORT int vfm_rectify_bayer(int ncam, const vfm_rectify_camera* cams_host, void* ws, size_t ws_bytes, vfm_stream_t stream) {
    size_t need = 0;
    VFM_TRY(rectify_check(ncam, cams_host, &need));
    VFM_CHECK_ARG(need == 0 || (ws && ws_bytes >= need), "rectify: workspace of %zu bytes needed (got %zu)", need, ws_bytes);
    RectifyArgs full, half;
    memset(&full, 0, sizeof(full));
    memset(&half, 0, sizeof(half));
    VfmCarver carve(ws);
    unsigned nfull = 0, nhalf = 0;
    for (int c = 0; c < ncam; ++c) {
        const vfm_rectify_camera& h = cams_host[c];
        VFM_CHECK_ARG(h.mosaic && h.table && h.out, "rectify: camera %d: null pointer", c);
        VFM_CHECK_ARG((reinterpret_cast<uintptr_t>(h.table) & 15u) == 0, "rectify: camera %d: the look-up table must be 16-byte aligned", c);
        RectifyCam d;
        d.mosaic = h.mosaic;
        d.table = reinterpret_cast<const double2*>(h.table);
        d.H = (int)h.H;
        d.W = (int)h.W;
        d.Hc = (int)(h.H - h.crop_bottom);
        d.code = bayer_code(h.pattern);
        d.full = h.subsample == 2 ? carve.take<uint8_t>((size_t)3 * d.Hc * d.W) : h.out;
        d.half = h.subsample == 2 ? h.out : nullptr;
        d.block0 = nfull;
        nfull += blocks_of((int64_t)d.Hc * d.W);
        full.cam[full.ncam++] = d;
        if (h.subsample == 2) {
            d.block0 = nhalf;
            nhalf += blocks_of((int64_t)(d.Hc / 2) * (d.W / 2));
            half.cam[half.ncam++] = d;
        }
    }
    hipLaunchKernelGGL(rectify_bayer_kernel, dim3(nfull), dim3(256), 0, (hipStream_t)stream, full);
    VFM_CHECK_LAUNCH("rectify_bayer_kernel");
    if (nhalf) {
        hipLaunchKernelGGL(resize2_bilinear_kernel, dim3(nhalf), dim3(256), 0, (hipStream_t)stream, half);
        VFM_CHECK_LAUNCH("resize2_bilinear_kernel");
    }
    return VFM_OK;
}
