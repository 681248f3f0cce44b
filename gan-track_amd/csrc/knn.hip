// k-nearest-neighbour manifolds of the improved precision / recall metric (SG3/metrics/precision_recall.py:51-61):
//   sg2_knn_radii:        radii[i] = (k + 1)-th smallest dist(x_i, x_j) over j      (the reference's kthvalue)
//   sg2_manifold_member:  hit[i]   = any_j dist(probe_i, manifold_j) <= radii[j]    (its `<=` / any)
// Both are one fp16 "NT" GEMM rows x cols over d (4096 VGG features) whose result is never stored: the epilogue turns
// each tile of dot products into d2 = |a|^2 + |b|^2 - 2 a.b and keeps, per row, the k + 1 smallest d2 or
// one flag, in registers.  The GEMM is conv3x3_s2g_kernel's (conv3x3.hip) with plain [rows][d] operands:
//   * workgroup tile 256 rows x 256 columns, 8 waves of 128 x 64 (8 row fragments x 4 column fragments: 32 MFMAs and
//     12 ds_read_b128 per wave and K step of 32), one workgroup a CU; the model's own 256 x 128 tile with 4 waves and
//     two workgroups a CU is the same template (Geo<2>, SG2_KNN_WIDE=0).  The kernel is bound by the L2 -> LDS
//     fill: the narrow tile ran at the fill rate its 85 FLOP per staged byte allow (0.27 of the MFMA peak at
//     50 000 x 50 000 x 4096), the wide one stages 2/3 of the bytes per FLOP and reaches 0.43;
//   * both operands arrive by LDS-DMA (buffer_load ... lds), 64-byte K slices, the swz64 XOR on the source side, a
//     3-slot ring filled two steps ahead with one barrier per step; the ring runs on across the column tiles of a
//     workgroup, so a tile's epilogue overlaps the next tile's first loads;
//   * a workgroup keeps its 256 rows and walks the column tiles of its column split; the lanes (4) and waves (4 or
//     2) that share a row merge through LDS at the end, and the workgroup writes one partial per (split, row); a
//     second small kernel merges the splits.  Taking the k + 1 smallest of a multiset and OR-ing flags do not depend
//     on the order: bitwise reproducible without atomics or a zero-filled accumulator;
//   * XCD-aware order: workgroup i runs on XCD i % 8 and takes item (i % 8) * (grid / 8) + i / 8; items are ordered
//     8 row tiles x the splits, so the workgroups of one XCD that share a column panel (same split) or a row panel
//     (same row tile) read it within a few K steps of each other and meet in that XCD's L2.
// Rounding to fp16 (round16) is monotone: the radii pass selects on d2 and rounds the winner only; the membership pass
// compares d2 with a per-column threshold = the largest f32 d2 whose rounded distance is still <= radii[j] (found by
// bisection on the float's bits with the very expression it stands for, one thread per column).
#include "sg2_common.h"

#include <algorithm>
#include <cstdlib>

namespace sg2 {
namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// Tile geometry: 256 rows x (64 WN) columns, 2 x WN waves of 128 x 64.  WN = 2 is conv3x3_s2g_kernel's tile (four
// waves, two workgroups a CU); WN = 4 (eight waves, one workgroup a CU) moves 2/3 of the bytes per FLOP from L2 to LDS
// (512 instead of 768 slot rows per 256 x 256 x 32 products) with 4 instead of 6 DMA instructions per wave and step.
constexpr int N_BM = 256, N_NS = 3;
constexpr int N_MAXSPLITS = 64;
// what the epilogue keeps: the k + 1 smallest d2 per row, one flag per row, or a count per row and a flag per column
constexpr int M_RADII = 0, M_MEMBER = 1, M_COUNT = 2;
template <int WN> struct Geo {
    static constexpr int BN = 64 * WN;                      // columns per tile
    static constexpr int NW = 2 * WN;                       // waves
    static constexpr int SLOT = (N_BM + BN) * 64;           // 24 / 32 KiB
    static constexpr int DMA = (N_BM + BN) / 16 / NW;       // wave-instructions per wave and step (6 / 4)
    static constexpr int ADMA = N_BM / 16 / NW;             // of which row-panel rows (4 / 2)
    static constexpr int SRC = 4 * WN;                      // (lane group, wave) pairs that share a row
    static constexpr size_t RING = (size_t)N_NS * SLOT;
    static constexpr size_t lds(int kl, int mode) {         // the ring, reused by the end-of-kernel merge
        const size_t merge = (size_t)N_BM * SRC * (mode == M_MEMBER ? 1 : mode == M_COUNT ? sizeof(int) : kl * sizeof(float));
        // (counting: 64 bytes behind the ring carry a tile's column flags from the lower to the upper row half)
        return (merge > RING ? merge : RING) + (mode == M_COUNT ? 64 : 0);
    }
};

template <int N>
__device__ __forceinline__ void wait_vm() {           // s_waitcnt vmcnt(N) (gfx9 encoding), expcnt / lgkmcnt untouched
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// v into the ascending list L (the largest of the KL + 1 values drops out)
template <int KL>
__device__ __forceinline__ void list_insert(float (&L)[KL], float v) {
#pragma unroll
    for (int i = 0; i < KL; ++i) {
        const float lo = fminf(L[i], v);
        v = fmaxf(L[i], v);
        L[i] = lo;
    }
}

struct KnnArgs {
    const void* rows;       // [nrows][d] fp16: the panel a workgroup keeps (radii: x, membership: the probes)
    const void* cols;       // [ncols][d] fp16: the panel it walks (radii: x, membership: the manifold)
    const float* nrow;      // [rows_pad] squared norms
    const float* ncol;      // [>= col_tiles * 128] squared norms, +inf past ncols in the radii pass
    const float* thr;       // membership, counting: [>= col_tiles * 128] d2 thresholds, -inf past ncols
    void* part;             // radii: float [splits][rows_pad][KL]; membership: uint32 [splits][rows_pad];
                            // counting: int32 [splits][rows_pad]
    uint8_t* colpart;       // counting: [row_tiles][cols_pad] column flags, one per (row tile, column)
    int nrows, ncols, d;
    int row_tiles, col_tiles, tiles_per_split, splits;
    int64_t rows_pad, cols_pad;
};

template <int KL, int MODE, int WN>
__global__ __launch_bounds__(128 * WN, 4 / WN) void knn_gemm_kernel(KnnArgs a) {
    typedef Geo<WN> G;
    constexpr bool MEMBER = MODE == M_MEMBER, COUNT = MODE == M_COUNT;
    constexpr int N_BN = G::BN, N_SLOT = G::SLOT, N_DMA = G::DMA, N_ADMA = G::ADMA, NW = G::NW, SRC = G::SRC;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, q = lane >> 4;
    const int t = (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8);
    const int per_group = 8 * a.splits;
    const int rem = t % per_group;
    const int rt = (t / per_group) * 8 + (rem & 7), sp = rem >> 3;
    if (rt >= a.row_tiles) return;
    const int m0 = rt * N_BM;
    const int ct0 = sp * a.tiles_per_split, ct1 = min(ct0 + a.tiles_per_split, a.col_tiles);
    const int nk = (a.d + 31) / 32;
    const int nsteps = (ct1 - ct0) * nk;
    const __amdgpu_buffer_rsrc_t rrb = make_rsrc(a.rows, (int64_t)a.nrows * a.d * 2);
    const __amdgpu_buffer_rsrc_t rcb = make_rsrc(a.cols, (int64_t)a.ncols * a.d * 2);

    // DMA lanes: instruction u of wave w fills slot rows (NW u + w) * 16 + lane / 4, piece lane % 4 (u < N_ADMA: the
    // row panel, else the column tile); the lane reads source piece j = (lane % 4) ^ ((row >> 1) & 2), which is the
    // same for every u.  A row past the panel's end, or a piece past d (the K tail), gets offset -1: past the buffer
    // range, which reads zeros (sg2_common.h make_rsrc).
    const int pj = ((lane & 3) ^ ((lane >> 3) & 2)) * 8;        // first K element of the lane's piece within a step
    int abase[N_ADMA], crow[N_DMA - N_ADMA];
#pragma unroll
    for (int u = 0; u < N_DMA; ++u) {
        const int r = (u * NW + wave) * 16 + (lane >> 2);
        if (u < N_ADMA) {
            const int m = m0 + r;
            abase[u] = m < a.nrows ? (m * a.d + pj) * 2 : -1;
        } else {
            crow[u - N_ADMA] = r - N_BM;
        }
    }
    int i_ct = ct0, i_k = 0;                                    // the next step to issue
    auto issue = [&](int slot) {
        const bool kin = i_k * 32 + pj < a.d;
        char* sb = smem_raw + slot * N_SLOT;
#pragma unroll
        for (int u = 0; u < N_DMA; ++u) {
            int off;
            if (u < N_ADMA) {
                off = (kin && abase[u] >= 0) ? abase[u] + i_k * 64 : -1;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rrb, (lds_ptr_t)(sb + (u * NW + wave) * 1024), 16, off, 0, 0, 0);
            } else {
                const int c = i_ct * N_BN + crow[u - N_ADMA];
                off = (kin && c < a.ncols) ? (c * a.d + pj) * 2 + i_k * 64 : -1;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rcb, (lds_ptr_t)(sb + (u * NW + wave) * 1024), 16, off, 0, 0, 0);
            }
        }
        if (++i_k == nk) { i_k = 0; ++i_ct; }
    };

    const int wm = wave / WN, wn = wave % WN;
    const int sw = ((q ^ ((l16 >> 1) & 2)) << 4) + l16 * 64;    // a fragment row's lane offset (row base % 16 == 0)
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane (l16, q) holds, per row fragment jp, row m0 + wm * 128 + 16 jp + l16 against the tile's columns
    // wn * 64 + 16 jc + 4 q + r (jc < 4, r < 4): 16 of a row's entries per tile
    float nr[8];
#pragma unroll
    for (int jp = 0; jp < 8; ++jp) nr[jp] = a.nrow[m0 + wm * 128 + jp * 16 + l16];
    float L[8][KL];                                             // radii: the running k + 1 smallest d2, ascending
    unsigned hit = 0;                                           // membership: bit jp
    int cnt[8];                                                 // counting: columns within their radius, per row
#pragma unroll
    for (int jp = 0; jp < 8; ++jp) cnt[jp] = 0;
#pragma unroll
    for (int jp = 0; jp < 8; ++jp)
#pragma unroll
        for (int i = 0; i < KL; ++i) L[jp][i] = __builtin_inff();

#pragma unroll
    for (int st = 0; st < N_NS - 1; ++st)
        if (st < nsteps) issue(st);
    int ct = ct0, kk = 0;
    for (int step = 0; step < nsteps; ++step) {
        if (step + N_NS - 2 < nsteps) wait_vm<(N_NS - 2) * N_DMA>();
        else wait_vm<0>();
        __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();                 // every wave's DMAs of this step landed; the oldest slot is free
        if (step + N_NS - 1 < nsteps) issue((step + N_NS - 1) % N_NS);
        const char* sb = smem_raw + (step % N_NS) * N_SLOT + sw;
        f16x8 cf[4], rf[8];
#pragma unroll
        for (int jc = 0; jc < 4; ++jc) cf[jc] = *(const f16x8*)(sb + (N_BM + wn * 64 + jc * 16) * 64);
#pragma unroll
        for (int jp = 0; jp < 8; ++jp) rf[jp] = *(const f16x8*)(sb + (wm * 128 + jp * 16) * 64);
#pragma unroll
        for (int jp = 0; jp < 8; ++jp)
#pragma unroll
            for (int jc = 0; jc < 4; ++jc)
                acc[jc][jp] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cf[jc], rf[jp], acc[jc][jp], 0, 0, 0);
        if (++kk < nk) continue;

        // ---- the tile's epilogue: acc[jc][jp][r] = row (jp, l16) . column ct * 128 + wn * 64 + 16 jc + 4 q + r ----
        const int colb = ct * N_BN + wn * 64 + 4 * q;
        float4 nb[4], th[4];
#pragma unroll
        for (int jc = 0; jc < 4; ++jc) {
            nb[jc] = *(const float4*)(a.ncol + colb + jc * 16);
            th[jc] = MEMBER || COUNT ? *(const float4*)(a.thr + colb + jc * 16) : float4{0.f, 0.f, 0.f, 0.f};
        }
        // radii: rows and columns are the same points; the tile holds diagonal entries if the ranges overlap
        const bool diag = MODE == M_RADII && ct * N_BN < m0 + N_BM && ct * N_BN + N_BN > m0;
        unsigned cmask = 0;                           // counting: bit 4 jc + r, the lane's 16 columns over its 8 rows
#pragma unroll
        for (int jp = 0; jp < 8; ++jp) {
            const int row = m0 + wm * 128 + jp * 16 + l16;
            unsigned rbits = 0;                       // counting: this row's 16 flags, bit 4 jc + r
#pragma unroll
            for (int jc = 0; jc < 4; ++jc) {
                const float nbv[4] = {nb[jc].x, nb[jc].y, nb[jc].z, nb[jc].w};
                const float thv[4] = {th[jc].x, th[jc].y, th[jc].z, th[jc].w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float d2 = fmaf(-2.f, acc[jc][jp][r], nr[jp] + nbv[r]);
                    if (MEMBER) {
                        // (the clamp at 0 cannot change d2 <= thr: thr is >= 0 or -inf)
                        hit |= d2 <= thv[r] ? 1u << jp : 0u;
                    } else if (COUNT) {
                        // (a row past nrows has a NaN norm: d2 is NaN and the comparison false for every threshold)
                        rbits |= d2 <= thv[r] ? 1u << (jc * 4 + r) : 0u;
                    } else {
                        if (diag && row == colb + jc * 16 + r) d2 = 0.f;
                        if (d2 < L[jp][KL - 1]) list_insert<KL>(L[jp], fmaxf(d2, 0.f));
                    }
                    acc[jc][jp][r] = 0.f;
                }
            }
            if (COUNT) {
                cnt[jp] += __builtin_popcount(rbits);
                cmask |= rbits;
            }
        }
        if (COUNT) {
            // the 16 lanes of a wave and the 2 waves (wm) that hold the same 16 columns: OR over the lanes by a
            // butterfly, over the waves through 2 bytes of LDS behind the ring.  Every wave of the workgroup ends
            // its tiles at the same step, so all of them meet at this barrier; the step barrier of the next tile
            // lies between this read and the next write.  Lane l16 < 4 of the upper wave then stores the four flags
            // of column fragment jc = l16 as one word: one partial per (row tile, column).
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) cmask |= (unsigned)__shfl_xor((int)cmask, off, 64);
            unsigned short* lc = (unsigned short*)(smem_raw + G::RING);
            if (wm == 1 && l16 == 0) lc[wn * 4 + q] = (unsigned short)cmask;
            __syncthreads();                          // (with its fences: these are plain LDS accesses, not DMA)
            if (wm == 0 && l16 < 4) {
                const unsigned nib = (cmask | lc[wn * 4 + q]) >> (l16 * 4);
                const unsigned word = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
                *(unsigned*)(a.colpart + (int64_t)rt * a.cols_pad + colb + l16 * 16) = word;
            }
        }
        kk = 0;
        ++ct;
    }
    wait_vm<0>();                                     // no LDS-DMA may outlive the workgroup
    __syncthreads();                                  // every wave is done with the ring: reuse it for the merge

    // ---- the 4 lanes x WN waves that share a row merge through LDS; thread tid < 256 then owns row m0 + tid ----
    const int src = wn * 4 + q;
    if (MEMBER) {
        unsigned char* lm = (unsigned char*)smem_raw;             // [256][SRC]
#pragma unroll
        for (int jp = 0; jp < 8; ++jp) lm[(wm * 128 + jp * 16 + l16) * SRC + src] = (hit >> jp) & 1;
        __syncthreads();
        if (tid >= N_BM) return;
        unsigned v = 0;
#pragma unroll
        for (int s = 0; s < SRC; s += 4) v |= *(const unsigned*)(lm + tid * SRC + s);
        ((unsigned*)a.part)[(int64_t)sp * a.rows_pad + m0 + tid] = v ? 1u : 0u;
    } else if (COUNT) {
        int* lm = (int*)smem_raw;                                 // [256][SRC]
#pragma unroll
        for (int jp = 0; jp < 8; ++jp) lm[(wm * 128 + jp * 16 + l16) * SRC + src] = cnt[jp];
        __syncthreads();
        if (tid >= N_BM) return;
        int v = 0;
#pragma unroll
        for (int s = 0; s < SRC; ++s) v += lm[tid * SRC + s];
        ((int*)a.part)[(int64_t)sp * a.rows_pad + m0 + tid] = v;
    } else {
        float* lm = (float*)smem_raw;                             // [256][SRC][KL]
#pragma unroll
        for (int jp = 0; jp < 8; ++jp)
#pragma unroll
            for (int i = 0; i < KL; ++i) lm[((wm * 128 + jp * 16 + l16) * SRC + src) * KL + i] = L[jp][i];
        __syncthreads();
        if (tid >= N_BM) return;
        float M[KL];
#pragma unroll
        for (int i = 0; i < KL; ++i) M[i] = __builtin_inff();
        for (int s = 0; s < SRC; ++s)
#pragma unroll
            for (int i = 0; i < KL; ++i) list_insert<KL>(M, lm[(tid * SRC + s) * KL + i]);
        float* o = (float*)a.part + ((int64_t)sp * a.rows_pad + m0 + tid) * KL;
#pragma unroll
        for (int i = 0; i < KL; ++i) o[i] = M[i];
    }
}

// out[row] = sum of x[row][:]^2 in f32 for row < n, `pad` for n <= row < n_pad.  One wave per row: lane l adds the
// 8-element pieces l, l + 64, ... in order, then the lanes' sums are added by a fixed butterfly.
__global__ __launch_bounds__(256) void knn_norm_kernel(float* out, const f16_t* x, int64_t n, int64_t n_pad, int d,
                                                       float pad) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_pad) return;
    if (row >= n) {
        if (lane == 0) out[row] = pad;
        return;
    }
    const f16x8* p = (const f16x8*)(x + row * d);
    float s = 0.f;
    for (int c = lane; c < d / 8; c += 64) {
        const f16x8 v = p[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf((float)v[e], (float)v[e], s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[row] = s;
}

__device__ __forceinline__ float knn_dist(float d2, int round16) {
    const float v = sqrtf(d2);
    return round16 ? (float)(f16_t)v : v;
}

// thr[j] = the largest f32 t >= 0 with knn_dist(t) <= radii[j] (dist is monotone in t and non-negative floats are
// ordered like their bits: bisection); -inf (never matches) for a NaN or negative radius and past n.
__global__ __launch_bounds__(256) void knn_thr_kernel(float* thr, const float* radii, int64_t n, int64_t n_pad,
                                                      int round16) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pad) return;
    float out = -__builtin_inff();
    if (j < n) {
        const float r = radii[j];
        if (r >= 0.f) {
            unsigned lo = 0u, hi = 0x7f800000u;           // dist(0) = 0 <= r holds; hi: +inf
            if (knn_dist(__builtin_inff(), round16) <= r) {
                lo = hi;
            } else {
                while (hi - lo > 1u) {
                    const unsigned mid = lo + ((hi - lo) >> 1);
                    if (knn_dist(__builtin_bit_cast(float, mid), round16) <= r) lo = mid;
                    else hi = mid;
                }
            }
            out = __builtin_bit_cast(float, lo);
        }
    }
    thr[j] = out;
}

template <int KL>
__global__ __launch_bounds__(256) void knn_merge_radii_kernel(float* radii, const float* part, int64_t n,
                                                              int64_t rows_pad, int splits, int k, int round16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float M[KL];
#pragma unroll
    for (int e = 0; e < KL; ++e) M[e] = __builtin_inff();
    for (int s = 0; s < splits; ++s) {
        const float* p = part + ((int64_t)s * rows_pad + i) * KL;
#pragma unroll
        for (int e = 0; e < KL; ++e) list_insert<KL>(M, p[e]);
    }
    float v = M[0];
#pragma unroll
    for (int e = 1; e < KL; ++e) v = e == k ? M[e] : v;
    radii[i] = knn_dist(v, round16);
}

__global__ __launch_bounds__(256) void knn_merge_hit_kernel(uint8_t* hit, const unsigned* part, int64_t p,
                                                            int64_t rows_pad, int splits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p) return;
    unsigned v = 0;
    for (int s = 0; s < splits; ++s) v |= part[(int64_t)s * rows_pad + i];
    hit[i] = v ? 1 : 0;
}

// count[i] = the sum of row i's partials over the splits; covered[j] = the OR of column j's partials over the row tiles
__global__ __launch_bounds__(256) void knn_merge_count_kernel(int32_t* count, uint8_t* covered, const int* part,
                                                              const uint8_t* colpart, int64_t p, int64_t n,
                                                              int64_t rows_pad, int64_t cols_pad, int splits,
                                                              int row_tiles) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < p) {
        int v = 0;
        for (int s = 0; s < splits; ++s) v += part[(int64_t)s * rows_pad + i];
        count[i] = v;
    }
    if (i < n) {
        unsigned v = 0;
        for (int t = 0; t < row_tiles; ++t) v |= colpart[(int64_t)t * cols_pad + i];
        covered[i] = v ? 1 : 0;
    }
}

// ---- host side ----
int num_cus() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            n = 256;
        }
        return n;
    }();
    return cus;
}

// SG2_KNN_WIDE (read per call; an A/B switch): 1 = the 256 x 256 tile (the default, the measured best), 0 = 256 x 128
bool wide_tile() {
    const char* e = getenv("SG2_KNN_WIDE");
    return !e || atoi(e) != 0;
}

struct KnnPlan {
    bool wide;
    int row_tiles, col_tiles, tiles_per_split, splits;
    int64_t rows_pad, cols_pad;
    // scratch layout in floats: nrow [rows_pad] | ncol [cols_pad] | thr [cols_pad] | part [splits][rows_pad][per_row]
    int64_t off_ncol, off_thr, off_part;
    int64_t bytes(int per_row) const { return (off_part + (int64_t)splits * rows_pad * per_row) * 4; }
};

// Column splits: the grid (row tiles x splits) should fill the machine's workgroup slots (2 a CU with the 256 x 128
// tile, 1 with the wide one) in whole rounds.  The
// smallest count that fills its last round to 95 %, else the best one; SG2_KNN_SPLITS overrides (read per call: the
// tests force several splits at small sizes).
KnnPlan make_plan(int64_t rows, int64_t cols) {
    KnnPlan p;
    p.wide = wide_tile();
    p.row_tiles = (int)cdiv(rows, N_BM);
    p.col_tiles = (int)cdiv(cols, p.wide ? Geo<4>::BN : Geo<2>::BN);
    const int maxs = std::max(1, std::min(p.col_tiles, N_MAXSPLITS));
    int splits = 1;
    const char* e = getenv("SG2_KNN_SPLITS");
    if (e && atoi(e) > 0) {
        splits = std::min(atoi(e), maxs);
    } else {
        const int64_t slots = (p.wide ? 1 : 2) * (int64_t)num_cus();
        double best = -1.0;
        for (int s = 1; s <= maxs; ++s) {
            const int64_t g = (int64_t)p.row_tiles * s;
            const double fill = (double)g / (double)(cdiv(g, slots) * slots);
            if (fill > best + 1e-9) { best = fill; splits = s; }
            if (fill >= 0.95) break;
        }
    }
    p.tiles_per_split = (int)cdiv(p.col_tiles, splits);
    p.splits = (int)cdiv(p.col_tiles, p.tiles_per_split);     // no empty split
    p.rows_pad = (int64_t)p.row_tiles * N_BM;
    p.cols_pad = cdiv(cols, N_BM) * N_BM;
    p.off_ncol = p.rows_pad;
    p.off_thr = p.off_ncol + p.cols_pad;
    p.off_part = p.off_thr + p.cols_pad;
    return p;
}

constexpr int64_t kMaxOperand = 0x7fffffffLL;       // 32-bit buffer offsets (sg2_common.h make_rsrc)

template <int KL, int MODE, int WN>
int launch_gemm_wn(const KnnArgs& a, hipStream_t s, const char* what) {
    auto kern = knn_gemm_kernel<KL, MODE, WN>;
    constexpr size_t lds = Geo<WN>::lds(KL, MODE);
    static_assert(lds <= 160 * 1024, "LDS");
    static bool attr_set = false;   // benign race: idempotent attribute
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    const int64_t grid = cdiv(a.row_tiles, 8) * 8 * a.splits;
    kern<<<(unsigned)grid, 128 * WN, lds, s>>>(a);
    return launch_status(what);
}

template <int KL, int MODE>
int launch_gemm(const KnnArgs& a, bool wide, hipStream_t s, const char* what) {
    return wide ? launch_gemm_wn<KL, MODE, 4>(a, s, what) : launch_gemm_wn<KL, MODE, 2>(a, s, what);
}

int check_common(const char* what, int dtype, int d, const void* scratch) {
    const std::string w(what);
    SG2_CHECK(dtype == SG2_F16, w + ": dtype must be SG2_F16");
    SG2_CHECK(d > 0 && d % 8 == 0, w + ": d must be a positive multiple of 8");
    SG2_CHECK(((uintptr_t)scratch % 16) == 0, w + ": scratch must be 16-byte aligned");
    return 0;
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_knn_scratch_bytes(int64_t* bytes, int64_t rows, int64_t cols, int k) {
    SG2_CHECK(bytes, "sg2_knn_scratch_bytes: bytes must be non-null");
    SG2_CHECK(rows >= 1 && cols >= 1, "sg2_knn_scratch_bytes: rows and cols must be >= 1");
    SG2_CHECK(k >= 1 && k <= 7, "sg2_knn_scratch_bytes: k must be in 1..7");
    *bytes = make_plan(rows, cols).bytes(k <= 3 ? 4 : 8);
    return 0;
}

extern "C" int sg2_knn_radii(float* radii, const void* x, int dtype, int64_t n, int d, int k, int round16,
                             void* scratch, int64_t scratch_bytes, void* stream) {
    SG2_CHECK(radii && x && scratch, "sg2_knn_radii: radii, x and scratch must be non-null");
    if (int rc = check_common("sg2_knn_radii", dtype, d, scratch)) return rc;
    SG2_CHECK(k >= 1 && k <= 7, "sg2_knn_radii: k must be in 1..7");
    SG2_CHECK(n >= k + 1, "sg2_knn_radii: n must be >= k + 1");
    SG2_CHECK(n * (int64_t)d * 2 <= kMaxOperand, "sg2_knn_radii: x must be below 2 GiB (32-bit buffer offsets)");
    SG2_CHECK(((uintptr_t)x % 16) == 0, "sg2_knn_radii: x must be 16-byte aligned");
    const KnnPlan p = make_plan(n, n);
    const int kl = k <= 3 ? 4 : 8;
    SG2_CHECK(scratch_bytes >= p.bytes(kl), "sg2_knn_radii: scratch too small (sg2_knn_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    float* f = (float*)scratch;
    // one norm array serves as rows and columns: +inf past n keeps the padding columns out of every list
    knn_norm_kernel<<<(unsigned)cdiv(p.rows_pad, 4), 256, 0, s>>>(f, (const f16_t*)x, n, p.rows_pad, d,
                                                                 __builtin_inff());
    if (int rc = launch_status("sg2_knn_radii (norms)")) return rc;
    KnnArgs a{};
    a.rows = a.cols = x;
    a.nrow = a.ncol = f;
    a.part = f + p.off_part;
    a.nrows = a.ncols = (int)n;
    a.d = d;
    a.row_tiles = p.row_tiles; a.col_tiles = p.col_tiles; a.tiles_per_split = p.tiles_per_split; a.splits = p.splits;
    a.rows_pad = p.rows_pad;
    if (int rc = kl == 4 ? launch_gemm<4, M_RADII>(a, p.wide, s, "sg2_knn_radii")
                         : launch_gemm<8, M_RADII>(a, p.wide, s, "sg2_knn_radii"))
        return rc;
    const unsigned mb = (unsigned)cdiv(n, 256);
    if (kl == 4) knn_merge_radii_kernel<4><<<mb, 256, 0, s>>>(radii, f + p.off_part, n, p.rows_pad, p.splits, k, round16);
    else knn_merge_radii_kernel<8><<<mb, 256, 0, s>>>(radii, f + p.off_part, n, p.rows_pad, p.splits, k, round16);
    return launch_status("sg2_knn_radii (merge)");
}

extern "C" int sg2_manifold_member(uint8_t* hit, const void* probes, int64_t p_n, const void* manifold, int64_t n,
                                   const float* radii, int dtype, int d, int round16, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
    SG2_CHECK(hit && probes && manifold && radii && scratch,
              "sg2_manifold_member: hit, probes, manifold, radii and scratch must be non-null");
    if (int rc = check_common("sg2_manifold_member", dtype, d, scratch)) return rc;
    SG2_CHECK(p_n >= 1 && n >= 1, "sg2_manifold_member: p and n must be >= 1");
    SG2_CHECK(p_n * (int64_t)d * 2 <= kMaxOperand && n * (int64_t)d * 2 <= kMaxOperand,
              "sg2_manifold_member: probes and manifold must each be below 2 GiB (32-bit buffer offsets)");
    SG2_CHECK(((uintptr_t)probes % 16) == 0 && ((uintptr_t)manifold % 16) == 0,
              "sg2_manifold_member: probes and manifold must be 16-byte aligned");
    const KnnPlan p = make_plan(p_n, n);
    // (the flags need one word per (split, row); the bound is sg2_knn_scratch_bytes' smallest answer for this shape)
    SG2_CHECK(scratch_bytes >= p.bytes(4), "sg2_manifold_member: scratch too small (sg2_knn_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    float* f = (float*)scratch;
    knn_norm_kernel<<<(unsigned)cdiv(p.rows_pad, 4), 256, 0, s>>>(f, (const f16_t*)probes, p_n, p.rows_pad, d, 0.f);
    knn_norm_kernel<<<(unsigned)cdiv(p.cols_pad, 4), 256, 0, s>>>(f + p.off_ncol, (const f16_t*)manifold, n, p.cols_pad,
                                                                 d, 0.f);
    knn_thr_kernel<<<(unsigned)cdiv(p.cols_pad, 256), 256, 0, s>>>(f + p.off_thr, radii, n, p.cols_pad, round16);
    if (int rc = launch_status("sg2_manifold_member (norms)")) return rc;
    KnnArgs a{};
    a.rows = probes;
    a.cols = manifold;
    a.nrow = f;
    a.ncol = f + p.off_ncol;
    a.thr = f + p.off_thr;
    a.part = f + p.off_part;
    a.nrows = (int)p_n;
    a.ncols = (int)n;
    a.d = d;
    a.row_tiles = p.row_tiles; a.col_tiles = p.col_tiles; a.tiles_per_split = p.tiles_per_split; a.splits = p.splits;
    a.rows_pad = p.rows_pad;
    if (int rc = launch_gemm<1, M_MEMBER>(a, p.wide, s, "sg2_manifold_member")) return rc;
    knn_merge_hit_kernel<<<(unsigned)cdiv(p_n, 256), 256, 0, s>>>(hit, (const unsigned*)(f + p.off_part), p_n, p.rows_pad,
                                                                 p.splits);
    return launch_status("sg2_manifold_member (merge)");
}

// Counting (density / coverage, Naeem et al. 2020): the membership pass with a counting epilogue that also reduces along
// the rows.  Scratch: the membership layout with one int per (split, row), then uint8 [row_tiles][cols_pad] column flags.
extern "C" int sg2_manifold_count_scratch_bytes(int64_t* bytes, int64_t p_n, int64_t n) {
    SG2_CHECK(bytes, "sg2_manifold_count_scratch_bytes: bytes must be non-null");
    SG2_CHECK(p_n >= 1 && n >= 1, "sg2_manifold_count_scratch_bytes: p and n must be >= 1");
    const KnnPlan p = make_plan(p_n, n);
    *bytes = p.bytes(1) + (int64_t)p.row_tiles * p.cols_pad;
    return 0;
}

extern "C" int sg2_manifold_count(int32_t* count, uint8_t* covered, const void* probes, int64_t p_n,
                                  const void* manifold, int64_t n, const float* radii, int dtype, int d, int round16,
                                  void* scratch, int64_t scratch_bytes, void* stream) {
    SG2_CHECK(count && covered && probes && manifold && radii && scratch,
              "sg2_manifold_count: count, covered, probes, manifold, radii and scratch must be non-null");
    if (int rc = check_common("sg2_manifold_count", dtype, d, scratch)) return rc;
    SG2_CHECK(p_n >= 1 && n >= 1, "sg2_manifold_count: p and n must be >= 1");
    SG2_CHECK(p_n * (int64_t)d * 2 <= kMaxOperand && n * (int64_t)d * 2 <= kMaxOperand,
              "sg2_manifold_count: probes and manifold must each be below 2 GiB (32-bit buffer offsets)");
    SG2_CHECK(((uintptr_t)probes % 16) == 0 && ((uintptr_t)manifold % 16) == 0,
              "sg2_manifold_count: probes and manifold must be 16-byte aligned");
    const KnnPlan p = make_plan(p_n, n);
    SG2_CHECK(scratch_bytes >= p.bytes(1) + (int64_t)p.row_tiles * p.cols_pad,
              "sg2_manifold_count: scratch too small (sg2_manifold_count_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    float* f = (float*)scratch;
    // A probe row past p reads as zeros: with a norm of 0 its d2 would be |b|^2, inside the ball of any manifold row
    // with |b|^2 <= thr, and would set that column's flag.  Its norm is NaN instead: d2 is NaN, `<=` false.
    knn_norm_kernel<<<(unsigned)cdiv(p.rows_pad, 4), 256, 0, s>>>(f, (const f16_t*)probes, p_n, p.rows_pad, d,
                                                                 __builtin_nanf(""));
    knn_norm_kernel<<<(unsigned)cdiv(p.cols_pad, 4), 256, 0, s>>>(f + p.off_ncol, (const f16_t*)manifold, n, p.cols_pad,
                                                                 d, 0.f);
    knn_thr_kernel<<<(unsigned)cdiv(p.cols_pad, 256), 256, 0, s>>>(f + p.off_thr, radii, n, p.cols_pad, round16);
    if (int rc = launch_status("sg2_manifold_count (norms)")) return rc;
    KnnArgs a{};
    a.rows = probes;
    a.cols = manifold;
    a.nrow = f;
    a.ncol = f + p.off_ncol;
    a.thr = f + p.off_thr;
    a.part = f + p.off_part;
    a.colpart = (uint8_t*)(f + p.off_part + (int64_t)p.splits * p.rows_pad);
    a.nrows = (int)p_n;
    a.ncols = (int)n;
    a.d = d;
    a.row_tiles = p.row_tiles; a.col_tiles = p.col_tiles; a.tiles_per_split = p.tiles_per_split; a.splits = p.splits;
    a.rows_pad = p.rows_pad;
    a.cols_pad = p.cols_pad;
    if (int rc = launch_gemm<1, M_COUNT>(a, p.wide, s, "sg2_manifold_count")) return rc;
    knn_merge_count_kernel<<<(unsigned)cdiv(std::max(p_n, n), 256), 256, 0, s>>>(
        count, covered, (const int*)a.part, a.colpart, p_n, n, p.rows_pad, p.cols_pad, p.splits, p.row_tiles);
    return launch_status("sg2_manifold_count (merge)");
}
