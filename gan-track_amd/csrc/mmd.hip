// The polynomial-kernel MMD sums of the kernel inception distance (SG3/metrics/kernel_inception_distance.py:33-44):
//   per subset s of m generated rows x_i = gen[idx_gen[s][i]] and m real rows y_j = real[idx_real[s][j]], with
//   k(a, b) = (a.b / d + 1)^3,
//   sums[s] = ( sum_{i != j} k(x_i, x_j),  sum_{i != j} k(y_i, y_j),  sum_{i, j} k(x_i, y_j) )
// The reference builds the three m x m Gram matrices on the host in float32 numpy (x @ x.T, y @ y.T, x @ y.T), cubes and
// sums them.  Here no matrix exists: one exact-f32 MFMA GEMM per 128 x 128 tile of a Gram whose epilogue applies the
// kernel and reduces the tile to one f64 number.
//   * Gather: a tile's rows are read through the index tables (64-bit row addresses: idx * d * 4 bytes), 128 bytes of
//     a row per 8 lanes, so no [S, m, d] copy is made either.  Positions past m read the subset's last row (a valid
//     address) and are masked in the epilogue.
//   * Workgroup: 256 threads, tile 128 x 128, K step 32; wave (wm, wn) owns 64 x 64 = 2 x 2 accumulators of
//     v_mfma_f32_32x32x2_f32 (64 accumulator registers).  The f32-input MFMA is bit for bit a k-ordered f32 fma chain.
//   * LDS: per K step the two 128 x 32 f32 operand tiles, rows padded to 36 floats (144 B): a lane reads 16 bytes
//     (4 consecutive k of its row) per 32-row fragment and 8 k, the 16 lanes that ds_read_b128 serves together then sit
//     on 16 distinct bank quads; the 8 lanes of a ds_write_b128 group write one row's 128 contiguous bytes.  Lane
//     (r, h) holds k = 8 g + 4 h + c (c < 4) of row r; MFMA c of group g multiplies k = 8 g + c (h = 0) and
//     8 g + 4 + c (h = 1): both operands are permuted alike, so only the order of the chain's terms changes.
//     Two buffers (72 KiB, two workgroups a CU), global loads of step k + 1 in flight under the MFMAs of step k, one
//     barrier per step: 16 MFMAs (1024 cycles) per 4 ds_read_b128 and wave.
//   * XCD-aware order (knn.hip's): workgroup b runs on XCD b % 8 and takes item (b % 8) * (grid / 8) + b / 8, so the
//     64 workgroups an XCD holds at a time are neighbouring tiles of one subset that share row and column panels and
//     meet in that XCD's L2: 8.6 instead of 10.0 ms at S = 100, m = 1000, d = 2048.  The partials are
//     indexed by item, so the order changes no bit.
//   * Symmetry: the xx and yy Grams run their upper-triangle tiles (ti <= tj) only; the fold counts ti < tj twice.
//     The diagonal is left out by position (row == col on a diagonal tile), never by comparing indices or values.
//   * Reduction: `/ d`, `+ 1` and the cube are separately rounded f32 operations (float32 numpy's); every kernel value
//     is then widened and ALL additions are f64 -- no f32 partial sum at all.  Order: a lane adds its 64 values in
//     register order, a fixed butterfly over the wave, the four waves as (0 + 1) + (2 + 3), one f64 partial per tile
//     into `scratch`; the fold kernel (one wave per subset and Gram) has lane l add tiles l, l + 64, ... in order and
//     the same butterfly.  The order depends on (S, m) alone, there are no atomics: results are bitwise reproducible.
//     Scratch entries of the skipped lower-triangle tiles are neither written nor read.
#include "sg2_common.h"

namespace sg2 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int M_BT = 128;                       // tile rows = tile columns
constexpr int M_BK = 32;                        // K step
constexpr int M_LDR = M_BK + 4;                 // floats per LDS row
constexpr int M_TILE = M_BT * M_LDR;            // floats per operand tile
constexpr int M_THREADS = 256;
constexpr size_t M_LDS = (size_t)2 * 2 * M_TILE * sizeof(float);    // two buffers x two operands: 73 728 bytes

struct MmdArgs {
    const float* gen;
    const float* real;
    const int32_t* idx_gen;     // [S][m]
    const int32_t* idx_real;    // [S][m]
    double* part;               // [S][3][T][T]
    int S, m, d, T;
};

__device__ __forceinline__ double mmd_wave_sum(double v) {      // a fixed butterfly: every lane gets the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(M_THREADS, 2) void mmd_tile_kernel(MmdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* lds = (float*)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int TT = a.T * a.T;
    // XCD-aware order: workgroup b runs on XCD b % 8 and takes item (b % 8) * (grid / 8) + b / 8, so the workgroups
    // one XCD runs at a time are neighbouring tiles -- one subset's, sharing row and column panels -- and meet in its L2
    const unsigned item = (blockIdx.x % 8u) * (gridDim.x / 8u) + blockIdx.x / 8u;
    if (item >= (unsigned)a.S * 3u * (unsigned)TT) return;              // (the grid is rounded up to 8)
    const int s = (int)(item / (unsigned)(3 * TT));
    const int rem = (int)(item % (unsigned)(3 * TT));
    const int g = rem / TT, ti = (rem % TT) / a.T, tj = rem % a.T;      // g: 0 = xx, 1 = yy, 2 = xy
    if (g < 2 && ti > tj) return;                                       // (uniform: before any barrier)
    const int m0 = ti * M_BT, n0 = tj * M_BT;

    // staging: thread (pr, pc) moves floats pc .. pc + 3 of tile rows pr + 32 u (u < 4) of both operands
    const int pr = tid >> 3, pc = (tid & 7) * 4;
    const float* rp[2][4];
    {
        const float* ra = g == 1 ? a.real : a.gen;
        const float* rb = g == 0 ? a.gen : a.real;
        const int32_t* ia = (g == 1 ? a.idx_real : a.idx_gen) + (int64_t)s * a.m;
        const int32_t* ib = (g == 0 ? a.idx_gen : a.idx_real) + (int64_t)s * a.m;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = min(m0 + pr + 32 * u, a.m - 1), q = min(n0 + pr + 32 * u, a.m - 1);
            rp[0][u] = ra + (int64_t)ia[p] * a.d + pc;
            rp[1][u] = rb + (int64_t)ib[q] * a.d + pc;
        }
    }
    float4 st[2][4];
    auto gload = [&](int kk) {
        const bool in = kk * M_BK + pc < a.d;           // d % 4 == 0: a float4 is inside the row or past it as a whole
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int u = 0; u < 4; ++u)
                st[o][u] = in ? *(const float4*)(rp[o][u] + kk * M_BK) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto sstore = [&](int buf) {
        float* base = lds + buf * 2 * M_TILE + pr * M_LDR + pc;
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int u = 0; u < 4; ++u) *(float4*)(base + o * M_TILE + 32 * u * M_LDR) = st[o][u];
    };

    const int wm = wave >> 1, wn = wave & 1;
    const int l32 = lane & 31, h = lane >> 5;
    const int fa = (wm * 64 + l32) * M_LDR + h * 4;              // the lane's first fragment of the row operand
    const int fb = M_TILE + (wn * 64 + l32) * M_LDR + h * 4;     // ... of the column operand
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (a.d + M_BK - 1) / M_BK;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
        if (kk + 1 < nk) gload(kk + 1);
        const float* base = lds + (kk & 1) * 2 * M_TILE;
#pragma unroll
        for (int g8 = 0; g8 < M_BK / 8; ++g8) {
            float4 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = *(const float4*)(base + fa + i * 32 * M_LDR + g8 * 8);
                bf[i] = *(const float4*)(base + fb + i * 32 * M_LDR + g8 * 8);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float av[2] = {c == 0 ? af[0].x : c == 1 ? af[0].y : c == 2 ? af[0].z : af[0].w,
                                     c == 0 ? af[1].x : c == 1 ? af[1].y : c == 2 ? af[1].z : af[1].w};
                const float bv[2] = {c == 0 ? bf[0].x : c == 1 ? bf[0].y : c == 2 ? bf[0].z : bf[0].w,
                                     c == 0 ? bf[1].x : c == 1 ? bf[1].y : c == 2 ? bf[1].z : bf[1].w};
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        }
        if (kk + 1 < nk) sstore((kk + 1) & 1);      // the other buffer: every wave left it at the last barrier
        __syncthreads();
    }

    // ---- epilogue: acc[i][j][r] = row m0 + wm * 64 + 32 i + (r & 3) + 8 (r >> 2) + 4 h  .  column n0 + wn * 64 + 32 j + l32
    const float fd = (float)a.d;
    const bool diag = g < 2 && ti == tj;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + 32 * j + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = __fadd_rn(__fdiv_rn(acc[i][j][r], fd), 1.f);
                const float k = __fmul_rn(__fmul_rn(v, v), v);
                const bool on = row < a.m && col < a.m && !(diag && row == col);
                sum += on ? (double)k : 0.0;
            }
        }
    sum = mmd_wave_sum(sum);
    double* red = (double*)smem_raw;                // (the K loop ended on a barrier: the buffers are free)
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) a.part[item] = (red[0] + red[1]) + (red[2] + red[3]);
}

// sums[s][g] = the tiles of Gram g of subset s in a fixed order; an off-diagonal tile of xx / yy counts twice
__global__ __launch_bounds__(192) void mmd_fold_kernel(double* sums, const double* part, int T) {
    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int TT = T * T;
    const double* p = part + ((int64_t)blockIdx.x * 3 + g) * TT;
    double acc = 0.0;
    for (int it = lane; it < TT; it += 64) {
        const int ti = it / T, tj = it % T;
        if (g < 2 && ti > tj) continue;
        acc += (g < 2 && ti < tj) ? 2.0 * p[it] : p[it];
    }
    acc = mmd_wave_sum(acc);
    if (lane == 0) sums[(int64_t)blockIdx.x * 3 + g] = acc;
}

int mmd_plan(const char* what, int S, int m, int& T, int64_t& bytes) {
    const std::string w(what);
    SG2_CHECK(S >= 1, w + ": S must be >= 1");
    SG2_CHECK(m >= 2, w + ": m must be >= 2 (the estimator divides by m - 1)");
    T = (int)cdiv(m, M_BT);
    SG2_CHECK((int64_t)S * 3 * T * T <= 0x7ffffff8LL, w + ": S * 3 * ceil(m / 128)^2 tiles are too many for one launch");
    bytes = (int64_t)S * 3 * T * T * 8;
    return 0;
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_poly_mmd_scratch_bytes(int64_t* bytes, int S, int m) {
    SG2_CHECK(bytes, "sg2_poly_mmd_scratch_bytes: bytes must be non-null");
    int T;
    return mmd_plan("sg2_poly_mmd_scratch_bytes", S, m, T, *bytes) < 0 ? -1 : 0;
}

extern "C" int sg2_poly_mmd_sums(double* sums, const float* gen, int64_t n_gen, const float* real, int64_t n_real,
                                 const int32_t* idx_gen, const int32_t* idx_real, int S, int m, int d, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
    SG2_CHECK(sums && gen && real && idx_gen && idx_real && scratch,
              "sg2_poly_mmd_sums: sums, gen, real, idx_gen, idx_real and scratch must be non-null");
    SG2_CHECK(d >= 4 && d % 4 == 0, "sg2_poly_mmd_sums: d must be a positive multiple of 4 (16-byte rows)");
    int T;
    int64_t need;
    if (mmd_plan("sg2_poly_mmd_sums", S, m, T, need) < 0) return -1;
    SG2_CHECK(n_gen >= 1 && n_real >= 1, "sg2_poly_mmd_sums: n_gen and n_real must be >= 1");
    SG2_CHECK(((uintptr_t)gen % 16) == 0 && ((uintptr_t)real % 16) == 0 && ((uintptr_t)scratch % 16) == 0,
              "sg2_poly_mmd_sums: gen, real and scratch must be 16-byte aligned");
    SG2_CHECK(((uintptr_t)sums % 8) == 0 && ((uintptr_t)idx_gen % 4) == 0 && ((uintptr_t)idx_real % 4) == 0,
              "sg2_poly_mmd_sums: sums must be 8-byte, the index tables 4-byte aligned");
    SG2_CHECK(scratch_bytes >= need, "sg2_poly_mmd_sums: scratch too small (sg2_poly_mmd_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    static bool attr_set = false;   // benign race: idempotent attribute
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)mmd_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)M_LDS);
        attr_set = true;
    }
    MmdArgs a;
    a.gen = gen; a.real = real; a.idx_gen = idx_gen; a.idx_real = idx_real;
    a.part = (double*)scratch;
    a.S = S; a.m = m; a.d = d; a.T = T;
    mmd_tile_kernel<<<(unsigned)(cdiv((int64_t)S * 3 * T * T, 8) * 8), M_THREADS, M_LDS, s>>>(a);
    if (int rc = launch_status("sg2_poly_mmd_sums")) return rc;
    mmd_fold_kernel<<<(unsigned)S, 192, 0, s>>>(sums, (const double*)scratch, T);
    return launch_status("sg2_poly_mmd_sums (fold)");
}
