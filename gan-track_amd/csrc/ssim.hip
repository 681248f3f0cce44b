// Structural similarity (Wang, Bovik, Sheikh, Simoncelli 2004, the original formulation) and mean squared error of a
// batch of image pairs in one pass over the two images:
//   w = g g^T, g[k] ~ exp(-(k - 5)^2 / (2 1.5^2)), k = 0..10, sum 1; valid positions only, (H - 10) x (W - 10)
//   mx = sum w x, my = sum w y, sxx = sum w x^2 - mx^2, syy = sum w y^2 - my^2, sxy = sum w x y - mx my
//   ssim = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),  C1 = (0.01 L)^2, C2 = (0.03 L)^2
//   out[i][0] = mean of ssim over the valid positions, out[i][1] = mean of (x - y)^2 over all H W pixels.
// In torch this is five depthwise convolutions and a dozen full-size temporaries; here the images are read once.
//   * Float64 throughout.  The inputs are f32, so x^2, y^2 and x y are exact in f64 (24 + 24 bits); the five moments
//     are fma chains in f64 and the map expression is evaluated in f64 without contraction.  sxx = E[x^2] - mx^2
//     cancels up to L^2 / C2 = 1111 times the moments' rounding into the map: f32 moments miss by 1e-5 on a flat image.
//   * One workgroup per 16 x 32 output tile and (n, c).  It stages the 26 x 42 pixels of x and y under the tile in LDS
//     (zeros outside the image), makes the horizontal pass into five f64 planes [26][32] of LDS (a thread per row and
//     column, 11 taps), then the vertical pass from those planes (a thread per output, 11 taps), evaluates the map and
//     stores it as f32 when asked.  Row-contiguous f64 planes: a half wave reads or writes 32 consecutive doubles, all
//     64 banks once; the f32 staging rows are read 32 consecutive floats at a time.  LDS: 8.5 + 32.5 + 4 KiB.
//   * The squared error is taken from the staged pixels: every pixel is owned by exactly one tile, the first 16 rows
//     and 32 columns of its staged block, and the last tile row and column also own their 10-pixel border.
//   * No atomics.  A tile's two sums (map, squared error) are reduced by a fixed tree over the 256 threads and written
//     to scratch [N C][tiles][2]; ssim_finalize_kernel adds an image's tiles in a fixed order (thread t takes tiles
//     t, t + 256, ..., then the same tree) and divides once.  The order depends on (H, W) alone: two calls give the
//     same bits, a pair gives the same bits alone or in a batch, and map == NULL changes nothing in out.  Every
//     scratch element that is read was written by the same call.
//   * x against itself: the xx, yy and xy chains are the same operations on the same bits and the expression is not
//     contracted, so numerator and denominator are equal bit for bit: the map is exactly 1.0 and so is its mean.
#include "sg2_common.h"

namespace sg2 {
namespace {

constexpr int SS_TAPS = 11;
constexpr int SS_HALO = SS_TAPS - 1;
constexpr int SS_TH = 16, SS_TW = 32;               // the output tile (torch_utils/ops/ssim.py TILE_H, TILE_W)
constexpr int SS_SH = SS_TH + SS_HALO, SS_SW = SS_TW + SS_HALO;
constexpr int SS_THREADS = 256;
constexpr int SS_MAX_HW = 1024;

struct SsimArgs {
    double* out;
    float* map;
    const float* x;
    const float* y;
    double* part;
    double g[SS_TAPS];
    double c1, c2;
    int64_t NC;
    int H, W, OH, OW, tiles_x, tiles;
};

// sums red[0][*] and red[1][*] into element 0: a fixed tree of depth 8
__device__ __forceinline__ void tree_sum2(double (*red)[SS_THREADS], int tid) {
    __syncthreads();
#pragma unroll
    for (int s = SS_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ double ssim_value(double ex, double ey, double exx, double eyy, double exy, double c1,
                                             double c2) {
#pragma clang fp contract(off)
    const double mxx = ex * ex, myy = ey * ey, mxy = ex * ey;
    const double sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
    const double num = (2.0 * mxy + c1) * (2.0 * sxy + c2);
    const double den = (mxx + myy + c1) * (sxx + syy + c2);
    return num / den;
}

__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(SsimArgs a) {
    __shared__ float sx[SS_SH * SS_SW], sy[SS_SH * SS_SW];
    __shared__ double hm[5][SS_SH][SS_TW];
    __shared__ double red[2][SS_THREADS];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, r0 = (tile / a.tiles_x) * SS_TH, c0 = (tile % a.tiles_x) * SS_TW;
    const int oh = min(SS_TH, a.OH - r0), ow = min(SS_TW, a.OW - c0);       // the tile's valid outputs
    const int sh = oh + SS_HALO, sw = ow + SS_HALO;                         // staged extent: r0 + sh <= H, c0 + sw <= W
    const int own_h = r0 + SS_TH >= a.OH ? sh : SS_TH, own_w = c0 + SS_TW >= a.OW ? sw : SS_TW;
    const int64_t plane = (int64_t)a.H * a.W, oplane = (int64_t)a.OH * a.OW;

    for (int64_t nc = blockIdx.y; nc < a.NC; nc += gridDim.y) {
        const float* px = a.x + nc * plane + (int64_t)r0 * a.W + c0;
        const float* py = a.y + nc * plane + (int64_t)r0 * a.W + c0;
        double se = 0.0;
        for (int i = tid; i < SS_SH * SS_SW; i += SS_THREADS) {
            const int r = i / SS_SW, c = i % SS_SW;
            float vx = 0.f, vy = 0.f;
            if (r < sh && c < sw) {
                vx = px[(int64_t)r * a.W + c];
                vy = py[(int64_t)r * a.W + c];
            }
            sx[i] = vx;
            sy[i] = vy;
            if (r < own_h && c < own_w) {
                const double d = (double)vx - (double)vy;
                se += d * d;
            }
        }
        __syncthreads();

        // horizontal pass: hm[m][r][c] = sum_k g[k] m(r, c + k), m = x, y, x^2, y^2, x y
        for (int i = tid; i < SS_SH * SS_TW; i += SS_THREADS) {
            const int r = i / SS_TW, c = i % SS_TW;
            double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
            for (int k = 0; k < SS_TAPS; ++k) {
                const double g = a.g[k];
                const double xv = (double)sx[r * SS_SW + c + k], yv = (double)sy[r * SS_SW + c + k];
                hx = fma(g, xv, hx);
                hy = fma(g, yv, hy);
                hxx = fma(g, xv * xv, hxx);
                hyy = fma(g, yv * yv, hyy);
                hxy = fma(g, xv * yv, hxy);
            }
            hm[0][r][c] = hx;
            hm[1][r][c] = hy;
            hm[2][r][c] = hxx;
            hm[3][r][c] = hyy;
            hm[4][r][c] = hxy;
        }
        __syncthreads();

        // vertical pass and the map: two outputs a thread
        double ms = 0.0;
#pragma unroll
        for (int j = 0; j < SS_TH * SS_TW / SS_THREADS; ++j) {
            const int i = tid + j * SS_THREADS, r = i / SS_TW, c = i % SS_TW;
            double ex = 0.0, ey = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
            for (int k = 0; k < SS_TAPS; ++k) {
                const double g = a.g[k];
                ex = fma(g, hm[0][r + k][c], ex);
                ey = fma(g, hm[1][r + k][c], ey);
                exx = fma(g, hm[2][r + k][c], exx);
                eyy = fma(g, hm[3][r + k][c], eyy);
                exy = fma(g, hm[4][r + k][c], exy);
            }
            const double s = ssim_value(ex, ey, exx, eyy, exy, a.c1, a.c2);
            if (r < oh && c < ow) {
                ms += s;
                if (a.map) a.map[nc * oplane + (int64_t)(r0 + r) * a.OW + c0 + c] = (float)s;
            }
        }
        red[0][tid] = ms;
        red[1][tid] = se;
        tree_sum2(red, tid);
        if (tid == 0) {
            double* p = a.part + (nc * a.tiles + tile) * 2;
            p[0] = red[0][0];
            p[1] = red[1][0];
        }
        __syncthreads();    // red and the staging are reused by the next (n, c)
    }
}

// out[nc] = (sum of the tiles' map sums / (OH OW), sum of their squared errors / (H W)), tiles in a fixed order
__global__ __launch_bounds__(SS_THREADS) void ssim_finalize_kernel(SsimArgs a) {
    __shared__ double red[2][SS_THREADS];
    const int tid = threadIdx.x;
    for (int64_t nc = blockIdx.x; nc < a.NC; nc += gridDim.x) {
        const double* p = a.part + nc * a.tiles * 2;
        double s0 = 0.0, s1 = 0.0;
        for (int t = tid; t < a.tiles; t += SS_THREADS) {
            s0 += p[2 * t];
            s1 += p[2 * t + 1];
        }
        red[0][tid] = s0;
        red[1][tid] = s1;
        tree_sum2(red, tid);
        if (tid == 0) {
            a.out[2 * nc] = red[0][0] / (double)((int64_t)a.OH * a.OW);
            a.out[2 * nc + 1] = red[1][0] / (double)((int64_t)a.H * a.W);
        }
        __syncthreads();
    }
}

int ssim_plan(const char* what, int N, int C, int H, int W, SsimArgs& a) {
    const std::string w(what);
    SG2_CHECK(N >= 1 && C >= 1, w + ": N and C must be >= 1");
    SG2_CHECK(H >= SS_TAPS && H <= SS_MAX_HW && W >= SS_TAPS && W <= SS_MAX_HW, w + ": H and W must be in 11..1024");
    a.NC = (int64_t)N * C;
    a.H = H;
    a.W = W;
    a.OH = H - SS_HALO;
    a.OW = W - SS_HALO;
    a.tiles_x = (int)cdiv(a.OW, SS_TW);
    a.tiles = a.tiles_x * (int)cdiv(a.OH, SS_TH);
    return 0;
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_ssim_scratch_bytes(int64_t* bytes, int N, int C, int H, int W) {
    SG2_CHECK(bytes, "sg2_ssim_scratch_bytes: bytes must be non-null");
    SsimArgs a;
    if (ssim_plan("sg2_ssim_scratch_bytes", N, C, H, W, a) < 0) return -1;
    *bytes = a.NC * a.tiles * 2 * (int64_t)sizeof(double);
    return 0;
}

extern "C" int sg2_ssim_mse(double* out, float* map, const float* x, const float* y, int N, int C, int H, int W,
                            const double* window11, double data_range, void* scratch, int64_t scratch_bytes,
                            void* stream) {
    SG2_CHECK(out && x && y && window11 && scratch,
              "sg2_ssim_mse: out, x, y, window11 and scratch must be non-null");
    SsimArgs a;
    if (ssim_plan("sg2_ssim_mse", N, C, H, W, a) < 0) return -1;
    SG2_CHECK(data_range > 0.0, "sg2_ssim_mse: data_range must be > 0");       // (false for NaN too)
    SG2_CHECK(scratch_bytes >= a.NC * a.tiles * 2 * (int64_t)sizeof(double),
              "sg2_ssim_mse: scratch too small (sg2_ssim_scratch_bytes)");
    SG2_CHECK(((uintptr_t)out % 8) == 0 && ((uintptr_t)scratch % 8) == 0 && ((uintptr_t)x % 4) == 0 &&
                  ((uintptr_t)y % 4) == 0 && ((uintptr_t)map % 4) == 0,
              "sg2_ssim_mse: out and scratch must be 8-byte, x, y and map 4-byte aligned");
    a.out = out;
    a.map = map;
    a.x = x;
    a.y = y;
    a.part = (double*)scratch;
    for (int k = 0; k < SS_TAPS; ++k) a.g[k] = window11[k];
    a.c1 = (0.01 * data_range) * (0.01 * data_range);
    a.c2 = (0.03 * data_range) * (0.03 * data_range);
    hipStream_t s = as_stream(stream);
    const unsigned planes = (unsigned)(a.NC < 65535 ? a.NC : 65535);
    ssim_tile_kernel<<<dim3((unsigned)a.tiles, planes), SS_THREADS, 0, s>>>(a);
    if (int rc = launch_status("sg2_ssim_mse (tiles)")) return rc;
    ssim_finalize_kernel<<<planes, SS_THREADS, 0, s>>>(a);
    return launch_status("sg2_ssim_mse (finalize)");
}
