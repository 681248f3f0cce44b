// The summed 2-D power spectrum of a batch of windowed, zero-padded images (SG3/avg_spectra.py:164-166, kept per
// channel and summed over the batch):
//   out[c, u, v] = sum_b | sum_{y, x} ((x[b, c, y, x] - mean[c]) / std[c]) w[y] w[x] exp(-2 pi i (u y + v x) / S) |^2,
//   S = N * interp, u, v in [0, S).
// The reference pads every N x N image to S x S, runs a float64 fftn and stores an S x S complex spectrum per image.
// Here it is a pruned DFT, two float64 GEMMs on v_mfma_f64_16x16x4_f64 whose K is N (the padding's zeros are never
// multiplied), and the only complex array that exists is the half-transformed T below.
//   * Twiddles: E[u, y] = tw[(u y) mod S] from one table of S complex f64 values that the caller computes (in more
//     than f64, conjugate-symmetric bit for bit: tw[S - k] = conj(tw[k]), tw[0] = 1, tw[S / 2] = -1).  Both kernels
//     copy the table to LDS (16 S bytes, 64 KiB at S = 4096) and gather from it; a lane walks its row of E with
//     idx += (4 u) mod S, one conditional subtract per K step, so no product exceeds S^2 <= 2^24.
//   * Row pass (spectrum_row_kernel): T[b, c, y, v] = sum_x Xw[y, x] E[v, x] for v < Vp = S / 2 + 1 rounded up to 32
//     (the input is real: the other columns follow from the Hermitian symmetry).  Real x complex, K = N.  A wave owns
//     32 y x 32 v (2 x 2 MFMA tiles, real and imaginary accumulators); its A operand is made while it is staged:
//     the pixel (uint8 or float32 through element strides) widened to f64, (p - mean) / std, times the rounded product
//     w[y] w[x] -- the reference's operations in the reference's order.  T goes to scratch as two f64 planes
//     [b c][re, im][N][Vp]; columns Vh .. Vp - 1 hold ordinary DFT values that the column pass multiplies and drops.
//   * Column pass (spectrum_col_kernel): a workgroup of four waves owns 128 u x 32 v of one channel and one batch
//     group, and loops over the group's images: F = E[u tile, :] T_b[:, v tile] as four real MFMAs per K step and
//     MFMA tile (Fr += Er Tr, Fr += (-Ei) Ti, Fi += Er Ti, Fi += Ei Tr), then P += Fr Fr + Fi Fi in f64 accumulators
//     that live across the batch loop.  The B operand is read straight from T (16 lanes = 128 contiguous bytes, the
//     four waves of a workgroup read the same lines), the A operand from the LDS table: 16 MFMAs of 16 x 16 x 4 per
//     four 8-byte loads and two 16-byte LDS reads, no barrier inside the loop.
//   * Batch groups: at S = 1024 and C = 1 there are only 32 x 17 wave tiles for 1024 SIMDs, so the batch is split
//     into G groups (a function of (B, C, N, interp) alone) and every group stores its tile of P once into scratch
//     [G][C][S][Vh].  spectrum_fold_kernel adds the groups in group order and writes every element of out exactly
//     once: v <= S / 2 from (u, v), v > S / 2 from ((S - u) % S, S - v).  No atomics; two calls give the same bits.
//     Every scratch element that is read was written by the same call.
#include "sg2_common.h"

namespace sg2 {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_S = 4096;
constexpr int SP_MAX_GROUPS = 16;
constexpr int SP_TARGET_WAVES = 2048;       // two waves a SIMD on 256 CUs

struct SpecPlan {
    int S, Vh, Vp, G, per;                  // per: images per batch group (the last group may hold fewer)
    int64_t t_bytes, p_bytes;
};

struct SpecArgs {
    double* out;
    const void* img;
    int64_t sb, sc, sy, sx;
    const double* window;
    const double* mean;
    const double* stdv;
    const double2* tw;
    double* T;
    double* P;
    int B, C, N, S, Vh, Vp, G, per;
};

__device__ __forceinline__ void load_table(double2* lds, const double2* tw, int S) {
    for (int i = threadIdx.x; i < S; i += SP_THREADS) lds[i] = tw[i];
    __syncthreads();
}

// T[bc][re, im][y][v] for a 64 y x 64 v workgroup tile; wave (wy, wv) owns 32 x 32
template <typename PixT>
__global__ __launch_bounds__(SP_THREADS) void spectrum_row_kernel(SpecArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2* tw = (double2*)smem_raw;
    load_table(tw, a.tw, a.S);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int bc = blockIdx.z, b = bc / a.C, c = bc % a.C;
    const int y0 = blockIdx.y * 64 + (wave >> 1) * 32, v0 = blockIdx.x * 64 + (wave & 1) * 32;
    if (y0 >= a.N || v0 >= a.Vp) return;                // (after the only barrier; uniform per wave)
    const double mean = a.mean[c], stdv = a.stdv[c];
    const PixT* img = (const PixT*)a.img + (int64_t)b * a.sb + (int64_t)c * a.sc;

    // A operand: lane (lr, lk) holds Xw[y0 + 16 i + lr][x = 4 ks + lk]
    int ya[2];
    double wy[2];
    bool yin[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = y0 + 16 * i + lr;
        yin[i] = y < a.N;
        ya[i] = yin[i] ? y : 0;
        wy[i] = a.window[ya[i]];
    }
    // B operand: lane (lr, lk) holds E[v0 + 16 j + lr][x = 4 ks + lk] = tw[(v x) mod S]
    int idx[2], step[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int vm = (v0 + 16 * j + lr) % a.S;
        idx[j] = (vm * lk) % a.S;
        step[j] = (4 * vm) % a.S;
    }
    f64x4 tr[2][2], ti[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) tr[i][j][r] = ti[i][j][r] = 0.0;

    for (int ks = 0; ks < a.N / 4; ++ks) {
        const int x = 4 * ks + lk;
        const double wx = a.window[x];
        double av[2];
        double2 e[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double p = (double)img[(int64_t)ya[i] * a.sy + (int64_t)x * a.sx];
            const double xw = ((p - mean) / stdv) * (wy[i] * wx);
            av[i] = yin[i] ? xw : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            e[j] = tw[idx[j]];
            idx[j] += step[j];
            idx[j] -= idx[j] >= a.S ? a.S : 0;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                tr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], e[j].x, tr[i][j], 0, 0, 0);
                ti[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], e[j].y, ti[i][j], 0, 0, 0);
            }
    }
    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
    const int64_t plane = (int64_t)a.N * a.Vp;
    double* T = a.T + (int64_t)bc * 2 * plane;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int v = v0 + 16 * j + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = y0 + 16 * i + lk + 4 * r;
                if (y < a.N && v < a.Vp) {
                    T[(int64_t)y * a.Vp + v] = tr[i][j][r];
                    T[plane + (int64_t)y * a.Vp + v] = ti[i][j][r];
                }
            }
        }
}

// P[g][c][u][v] = sum over the images of batch group g of |F_b[u, v]|^2; workgroup tile 128 u x 32 v, wave w owns
// u rows 32 w .. 32 w + 31
__global__ __launch_bounds__(SP_THREADS, 2) void spectrum_col_kernel(SpecArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2* tw = (double2*)smem_raw;
    load_table(tw, a.tw, a.S);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int c = blockIdx.z % a.C, g = blockIdx.z / a.C;
    const int u0 = blockIdx.y * 128 + wave * 32, v0 = blockIdx.x * 32;
    if (u0 >= a.S) return;                              // (after the only barrier; uniform per wave)
    const int b_lo = g * a.per, b_hi = min(a.B, b_lo + a.per);

    // A operand: lane (lr, lk) holds E[u0 + 16 i + lr][y = 4 ks + lk]; rows past S are computed and dropped
    int idx0[2], step[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int um = (u0 + 16 * i + lr) % a.S;
        idx0[i] = (um * lk) % a.S;
        step[i] = (4 * um) % a.S;
    }
    const int64_t plane = (int64_t)a.N * a.Vp;
    // B operand: lane (lr, lk) holds T[y = 4 ks + lk][v0 + 16 j + lr]; v0 + 31 < Vp always
    const int64_t boff = (int64_t)lk * a.Vp + v0 + lr;
    f64x4 pw[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) pw[i][j][r] = 0.0;

    for (int b = b_lo; b < b_hi; ++b) {
        const double* Tr = a.T + ((int64_t)b * a.C + c) * 2 * plane + boff;
        const double* Ti = Tr + plane;
        f64x4 fr[2][2], fi[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) fr[i][j][r] = fi[i][j][r] = 0.0;
        int idx[2] = {idx0[0], idx0[1]};
        double tr[2], ti[2];
        tr[0] = Tr[0]; tr[1] = Tr[16]; ti[0] = Ti[0]; ti[1] = Ti[16];
        const int nk = a.N / 4;
        for (int ks = 0; ks < nk; ++ks) {
            double2 e[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                e[i] = tw[idx[i]];
                idx[i] += step[i];
                idx[i] -= idx[i] >= a.S ? a.S : 0;
            }
            const double ctr[2] = {tr[0], tr[1]}, cti[2] = {ti[0], ti[1]};
            if (ks + 1 < nk) {                          // the next step's rows, in flight under this step's MFMAs
                const int64_t o = (int64_t)(ks + 1) * 4 * a.Vp;
                tr[0] = Tr[o]; tr[1] = Tr[o + 16]; ti[0] = Ti[o]; ti[1] = Ti[o + 16];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    fr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[i].x, ctr[j], fr[i][j], 0, 0, 0);
                    fr[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-e[i].y, cti[j], fr[i][j], 0, 0, 0);
                    fi[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[i].x, cti[j], fi[i][j], 0, 0, 0);
                    fi[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(e[i].y, ctr[j], fi[i][j], 0, 0, 0);
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pw[i][j][r] += fr[i][j][r] * fr[i][j][r] + fi[i][j][r] * fi[i][j][r];
    }
    double* P = a.P + ((int64_t)g * a.C + c) * a.S * a.Vh;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int v = v0 + 16 * j + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = u0 + 16 * i + lk + 4 * r;
                if (u < a.S && v < a.Vh) P[(int64_t)u * a.Vh + v] = pw[i][j][r];
            }
        }
}

// out[c][u][v] = the groups' P in group order; v > S / 2 takes the mirrored element.  One thread per element of out.
__global__ __launch_bounds__(SP_THREADS) void spectrum_fold_kernel(SpecArgs a) {
    const int64_t n = (int64_t)a.C * a.S * a.S;
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int v = (int)(i % a.S), u = (int)((i / a.S) % a.S), c = (int)(i / ((int64_t)a.S * a.S));
    const int su = v < a.Vh ? u : (a.S - u) % a.S, sv = v < a.Vh ? v : a.S - v;
    const int64_t gs = (int64_t)a.C * a.S * a.Vh;
    const double* p = a.P + ((int64_t)c * a.S + su) * a.Vh + sv;
    double acc = p[0];
    for (int g = 1; g < a.G; ++g) acc += p[g * gs];
    a.out[i] = acc;
}

int spectrum_plan(const char* what, int B, int C, int N, int interp, SpecPlan& p) {
    const std::string w(what);
    SG2_CHECK(B >= 1 && C >= 1, w + ": B and C must be >= 1");
    SG2_CHECK(N >= 8 && N <= 1024 && N % 4 == 0, w + ": N must be a multiple of 4 in 8..1024");
    SG2_CHECK(interp >= 1, w + ": interp must be >= 1");
    SG2_CHECK((int64_t)N * interp <= SP_MAX_S, w + ": S = N * interp must be <= 4096 (the twiddle table lives in LDS)");
    SG2_CHECK((int64_t)B * C <= 65535, w + ": B * C must be <= 65535 (one grid plane per image-channel)");
    p.S = N * interp;
    p.Vh = p.S / 2 + 1;
    p.Vp = (int)cdiv(p.Vh, 32) * 32;
    const int64_t wave_tiles = cdiv(p.S, 32) * (p.Vp / 32) * C;
    int64_t G = cdiv(SP_TARGET_WAVES, wave_tiles);
    G = G < 1 ? 1 : G;
    G = G > SP_MAX_GROUPS ? SP_MAX_GROUPS : G;
    G = G > B ? B : G;
    p.per = (int)cdiv(B, G);
    p.G = (int)cdiv(B, p.per);              // every group holds at least one image
    SG2_CHECK((int64_t)p.G * C <= 65535, w + ": C is too large for one launch");
    p.t_bytes = (int64_t)B * C * 2 * N * p.Vp * 8;
    p.p_bytes = (int64_t)p.G * C * p.S * p.Vh * 8;
    return 0;
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_power_spectrum_scratch_bytes(int64_t* bytes, int B, int C, int N, int interp) {
    SG2_CHECK(bytes, "sg2_power_spectrum_scratch_bytes: bytes must be non-null");
    SpecPlan p;
    if (spectrum_plan("sg2_power_spectrum_scratch_bytes", B, C, N, interp, p) < 0) return -1;
    *bytes = p.t_bytes + p.p_bytes;
    return 0;
}

extern "C" int sg2_power_spectrum_sum(double* out, const void* img, int dtype, const int64_t* strides, int B, int C,
                                      int N, int interp, const double* window, const double* mean, const double* std,
                                      const double* twiddle, void* scratch, int64_t scratch_bytes, void* stream) {
    SG2_CHECK(out && img && strides && window && mean && std && twiddle && scratch,
              "sg2_power_spectrum_sum: out, img, strides, window, mean, std, twiddle and scratch must be non-null");
    SG2_CHECK(dtype == SG2_F32 || dtype == SG2_U8, "sg2_power_spectrum_sum: dtype must be SG2_F32 or SG2_U8");
    SpecPlan p;
    if (spectrum_plan("sg2_power_spectrum_sum", B, C, N, interp, p) < 0) return -1;
    SG2_CHECK(((uintptr_t)out % 8) == 0 && ((uintptr_t)window % 8) == 0 && ((uintptr_t)mean % 8) == 0 &&
                  ((uintptr_t)std % 8) == 0 && ((uintptr_t)twiddle % 16) == 0 && ((uintptr_t)scratch % 16) == 0,
              "sg2_power_spectrum_sum: out, window, mean and std must be 8-byte, twiddle and scratch 16-byte aligned");
    SG2_CHECK(dtype != SG2_F32 || ((uintptr_t)img % 4) == 0, "sg2_power_spectrum_sum: float32 img must be 4-byte aligned");
    SG2_CHECK(scratch_bytes >= p.t_bytes + p.p_bytes,
              "sg2_power_spectrum_sum: scratch too small (sg2_power_spectrum_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    SpecArgs a;
    a.out = out; a.img = img;
    a.sb = strides[0]; a.sc = strides[1]; a.sy = strides[2]; a.sx = strides[3];
    a.window = window; a.mean = mean; a.stdv = std; a.tw = (const double2*)twiddle;
    a.T = (double*)scratch;
    a.P = (double*)((char*)scratch + p.t_bytes);
    a.B = B; a.C = C; a.N = N; a.S = p.S; a.Vh = p.Vh; a.Vp = p.Vp; a.G = p.G; a.per = p.per;
    const size_t lds = (size_t)p.S * 16;        // <= 64 KiB, the dynamic LDS a launch may ask for without an attribute
    const dim3 rg((unsigned)cdiv(p.Vp, 64), (unsigned)cdiv(N, 64), (unsigned)(B * C));
    if (dtype == SG2_F32) spectrum_row_kernel<float><<<rg, SP_THREADS, lds, s>>>(a);
    else spectrum_row_kernel<uint8_t><<<rg, SP_THREADS, lds, s>>>(a);
    if (int rc = launch_status("sg2_power_spectrum_sum (row pass)")) return rc;
    const dim3 cg((unsigned)(p.Vp / 32), (unsigned)cdiv(p.S, 128), (unsigned)(p.G * C));
    spectrum_col_kernel<<<cg, SP_THREADS, lds, s>>>(a);
    if (int rc = launch_status("sg2_power_spectrum_sum (column pass)")) return rc;
    spectrum_fold_kernel<<<(unsigned)cdiv((int64_t)C * p.S * p.S, SP_THREADS), SP_THREADS, 0, s>>>(a);
    return launch_status("sg2_power_spectrum_sum (fold)");
}
