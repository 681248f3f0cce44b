// The small-tensor part of a latent projection step (SG3/genlib/projector/projector.py:259-268 and :294-298):
//   sg2_noise_reg_fwd / _bwd:    reg = sum_buf sum_level mean(n roll_x n)^2 + mean(n roll_y n)^2 over a pyramid of 2x2
//                                average pools per noise buffer, and its gradient;
//   sg2_noise_normalize_multi:   per buffer x -= mean(x); x *= 1 / sqrt(mean(x^2)) in place.
// All noise buffers of a generator (13 at 256^2: 175k floats) live in ONE flat f32 buffer; a host table of
// (offset, R) rows names them.  The reference's composition is ~70 tiny launches per buffer and direction; here the
// work is latency-bound, so what counts is the number of launches and the dependency chain:
//   forward  = 3 launches: pool (every level of every buffer, one 16P x 16P tile a workgroup: the pools nest, so no
//              tile needs another tile's data) -> corr (every (buffer, level) in 1024-element chunks: the two circular
//              products and a workgroup sum; the shift crosses tiles, hence the pooled levels live in scratch) ->
//              finalize (one workgroup: per level the chunk partials, the means, the squares, their sum);
//   backward = 1 launch: a gather -- every level-0 element adds, over the levels, its ancestor's four circular
//              neighbours weighted by 4^-l 2 m / cnt_l, and is written once (assign or add);
//   normalize = 1 launch, a workgroup per buffer, three passes over L2-resident data.
// Every sum is a fixed tree (no atomics): <= 16-term serial runs per lane, wave butterflies, LDS across waves,
// then <= 16-term runs over chunk partials.  Two calls on the same input give the same bits.
// The *_batched entry points run the same kernel bodies over B samples per buffer (buffer-major: sample s of buffer b
// at off[b] + s R^2), the sample being the grid's y: the launch counts do not grow with B, every sample has its own
// share of the scratch, and a sample's results are bitwise those of the batch-1 entry points on its buffers alone.
#include "sg2_common.h"

namespace sg2 {
namespace {

constexpr int NR_MAXBUF = 32;
constexpr int NR_MAXBATCH = 64;     // samples of the batched entry points (a grid dimension)
constexpr int NR_CHUNK = 1024;      // elements per corr / bwd workgroup (256 threads x float4)
constexpr int NR_MAXLEV = 8;        // R = 1024: 1024, 512, ..., 8

struct NrArgs {
    int nbuf, nitems;               // items = (buffer, level) pairs
    int R[NR_MAXBUF];
    int nlev[NR_MAXBUF];
    int item0[NR_MAXBUF + 1];       // first item of a buffer
    int pool_blk[NR_MAXBUF + 1];    // first pool tile of a buffer
    int corr_blk[NR_MAXBUF + 1];    // first corr chunk of a buffer (its levels follow one another)
    int bwd_blk[NR_MAXBUF + 1];     // first level-0 chunk of a buffer
    int64_t off[NR_MAXBUF];         // the buffer in flat (floats)
    int64_t soff[NR_MAXBUF];        // its pooled levels 1.. in scratch (floats)
    int64_t part_off;               // the corr partials (float2 per chunk) in scratch (floats)
};

__host__ __device__ inline int nr_levels(int R) {       // evaluate; stop at size <= 8; else pool and repeat
    int n = 1;
    while (R > 8) { R >>= 1; ++n; }
    return n;
}
__host__ __device__ inline int64_t nr_level_off(int R, int l) {   // floats in front of pooled level l >= 1
    int64_t o = 0;
    for (int j = 1; j < l; ++j) o += (int64_t)(R >> j) * (R >> j);
    return o;
}
__host__ __device__ inline int nr_chunks(int S) { return (S * S + NR_CHUNK - 1) / NR_CHUNK; }

__device__ __forceinline__ int nr_find(const int* prefix, int nbuf, int blk) {   // prefix[b] <= blk < prefix[b + 1]
    int b = 0;
    while (b + 1 < nbuf && prefix[b + 1] <= blk) ++b;
    return b;
}

__device__ __forceinline__ float wave_sum(float v) {    // a fixed butterfly: every lane gets the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the workgroup's NW waves (NW a power of two <= 16), returned to every thread.  red: NW floats of LDS.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                    // red may still be read from the previous use
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) t[i] = red[i];
#pragma unroll
    for (int s = NW / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int i = 0; i < s; ++i) t[i] += t[i + s];
    return t[0];
}

// Every kernel body below is a device function of (argument block, workgroup index, sample): the batch-1 kernels call
// it with sample 0 and the batched ones with blockIdx.y and that sample's scratch, so both run one code and one tree.
// Sample s of buffer b lies at flat + off[b] + s R^2 (the buffer-major layout of make_batched_table).

// ---- pool: thread (ly, lx) of a 16 x 16 workgroup owns a P x P patch of level 0, pools it in registers down to one
// value (levels 1 .. log2 P), then the workgroup pools its 16 x 16 values through LDS (4 more levels).  P = 4 reaches
// level 6 (R <= 512), P = 8 level 7 (R = 1024).
template <int P>
__device__ __forceinline__ void nr_pool_body(const NrArgs& a, int blk, int64_t samp, const float* __restrict__ flat,
                                             float* __restrict__ scratch, float (*lds)[256]) {
    constexpr int TILE = 16 * P, KP = P == 4 ? 2 : 3;
    const int b = nr_find(a.pool_blk, a.nbuf, blk);
    const int t = blk - a.pool_blk[b];
    const int R = a.R[b], nlev = a.nlev[b];
    const int tiles_x = R > TILE ? R / TILE : 1;
    const int ty = t / tiles_x, tx = t % tiles_x;
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = tx * TILE + lx * P, y0 = ty * TILE + ly * P;
    const bool active = x0 < R && y0 < R;               // R >= 16 here: a multiple of P
    const float* src = flat + a.off[b] + samp * R * R;
    float* dst = scratch + a.soff[b];

    float v[P][P];
    if (active) {
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; j += 4) {
                const float4 q = *(const float4*)(src + (int64_t)(y0 + i) * R + x0 + j);
                v[i][j] = q.x; v[i][j + 1] = q.y; v[i][j + 2] = q.z; v[i][j + 3] = q.w;
            }
    } else {
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int j = 0; j < P; ++j) v[i][j] = 0.f;
    }
#pragma unroll
    for (int k = 1; k <= KP; ++k) {
        const int s = P >> k;                           // the patch's side at level k
#pragma unroll
        for (int i = 0; i < s; ++i)
#pragma unroll
            for (int j = 0; j < s; ++j)
                v[i][j] = ((v[2 * i][2 * j] + v[2 * i][2 * j + 1]) + (v[2 * i + 1][2 * j] + v[2 * i + 1][2 * j + 1])) * 0.25f;
        if (active && k < nlev) {
            const int S = R >> k;
            float* d = dst + nr_level_off(R, k) + (int64_t)(y0 >> k) * S + (x0 >> k);
#pragma unroll
            for (int i = 0; i < s; ++i)
#pragma unroll
                for (int j = 0; j < s; ++j) d[i * S + j] = v[i][j];
        }
    }
    lds[0][tid] = v[0][0];
#pragma unroll
    for (int u = 1; u <= 4; ++u) {
        const int k = KP + u, s = 16 >> u;              // the tile's side at level k
        __syncthreads();
        if (k >= nlev) break;                           // uniform: nlev is the buffer's
        if (tid < s * s) {
            const int i = tid / s, j = tid % s;
            const float* p = lds[(u - 1) & 1];
            const int ps = 2 * s;
            const float r = ((p[2 * i * ps + 2 * j] + p[2 * i * ps + 2 * j + 1]) +
                             (p[(2 * i + 1) * ps + 2 * j] + p[(2 * i + 1) * ps + 2 * j + 1])) * 0.25f;
            lds[u & 1][i * s + j] = r;
            const int S = R >> k;
            const int gy = ty * (TILE >> k) + i, gx = tx * (TILE >> k) + j;
            if (gy < S && gx < S) dst[nr_level_off(R, k) + (int64_t)gy * S + gx] = r;
        }
    }
}

template <int P>
__global__ __launch_bounds__(256) void nr_pool_kernel(NrArgs a, const float* __restrict__ flat,
                                                      float* __restrict__ scratch) {
    __shared__ float lds[2][256];
    nr_pool_body<P>(a, blockIdx.x, 0, flat, scratch, lds);
}

template <int P>    // grid (pool tiles, B); sstride: floats of scratch per sample
__global__ __launch_bounds__(256) void nr_pool_batched_kernel(NrArgs a, const float* __restrict__ flat,
                                                              float* __restrict__ scratch, int64_t sstride) {
    __shared__ float lds[2][256];
    nr_pool_body<P>(a, blockIdx.x, blockIdx.y, flat, scratch + blockIdx.y * sstride, lds);
}

// ---- corr: one 1024-element chunk of one level: sum n[y][x] n[y][x-1] and sum n[y][x] n[y-1][x] (circular) ----
__device__ __forceinline__ void nr_corr_body(const NrArgs& a, int blk, int64_t samp, const float* __restrict__ flat,
                                             float* __restrict__ scratch, float* red) {
    const int b = nr_find(a.corr_blk, a.nbuf, blk);
    int c = blk - a.corr_blk[b];
    const int R = a.R[b];
    int l = 0;
    while (c >= nr_chunks(R >> l)) { c -= nr_chunks(R >> l); ++l; }     // l < nlev: the prefix counts exactly these
    const int S = R >> l, m = S - 1, n = S * S;
    const float* p = l == 0 ? flat + a.off[b] + samp * R * R : scratch + a.soff[b] + nr_level_off(R, l);
    const int e = c * NR_CHUNK + (int)threadIdx.x * 4;
    float px = 0.f, py = 0.f;
    if (e < n) {                                        // S % 4 == 0: the four elements share a row
        const int y = e / S, x = e - y * S;
        const float4 o = *(const float4*)(p + e);
        const float4 u = *(const float4*)(p + ((y - 1) & m) * S + x);
        const float lf = p[y * S + ((x - 1) & m)];
        px = (o.x * lf + o.y * o.x) + (o.z * o.y + o.w * o.z);
        py = (o.x * u.x + o.y * u.y) + (o.z * u.z + o.w * u.w);
    }
    px = block_sum<4>(px, red);
    py = block_sum<4>(py, red);
    if (threadIdx.x == 0) *(float2*)(scratch + a.part_off + 2 * (int64_t)blk) = float2{px, py};
}

__global__ __launch_bounds__(256) void nr_corr_kernel(NrArgs a, const float* __restrict__ flat,
                                                      float* __restrict__ scratch) {
    __shared__ float red[4];
    nr_corr_body(a, blockIdx.x, 0, flat, scratch, red);
}

__global__ __launch_bounds__(256) void nr_corr_batched_kernel(NrArgs a, const float* __restrict__ flat,
                                                              float* __restrict__ scratch, int64_t sstride) {
    __shared__ float red[4];
    nr_corr_body(a, blockIdx.x, blockIdx.y, flat, scratch + blockIdx.y * sstride, red);
}

// ---- finalize: one workgroup of 16 waves; a wave per (buffer, level) sums that level's chunk partials ----
__device__ __forceinline__ void nr_finalize_body(const NrArgs& a, float* __restrict__ reg, float* __restrict__ means,
                                                 const float* __restrict__ scratch, float* term) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2* part = (const float2*)(scratch + a.part_off);
    for (int it = wave; it < a.nitems; it += 16) {
        const int b = nr_find(a.item0, a.nbuf, it);
        const int l = it - a.item0[b], R = a.R[b];
        int first = a.corr_blk[b];
        for (int j = 0; j < l; ++j) first += nr_chunks(R >> j);
        const int S = R >> l, nch = nr_chunks(S);
        float sx = 0.f, sy = 0.f;
        for (int j = lane; j < nch; j += 64) {          // <= 16 terms a lane (R = 1024, level 0)
            const float2 q = part[first + j];
            sx += q.x;
            sy += q.y;
        }
        sx = wave_sum(sx);
        sy = wave_sum(sy);
        const float cnt = (float)(S * S);
        const float mx = sx / cnt, my = sy / cnt;
        if (lane == 0) {
            *(float2*)(means + 2 * it) = float2{mx, my};
            term[it] = mx * mx + my * my;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
        for (int j = lane; j < a.nitems; j += 64) s += term[j];
        s = wave_sum(s);
        if (lane == 0) reg[0] = s;
    }
}

__global__ __launch_bounds__(1024) void nr_finalize_kernel(NrArgs a, float* __restrict__ reg, float* __restrict__ means,
                                                           const float* __restrict__ scratch) {
    __shared__ float term[NR_MAXBUF * NR_MAXLEV];
    nr_finalize_body(a, reg, means, scratch, term);
}

// grid (1, B): sample s writes reg[s] and means[s][nitems][2]
__global__ __launch_bounds__(1024) void nr_finalize_batched_kernel(NrArgs a, float* __restrict__ reg,
                                                                   float* __restrict__ means,
                                                                   const float* __restrict__ scratch, int64_t sstride) {
    __shared__ float term[NR_MAXBUF * NR_MAXLEV];
    const int64_t s = blockIdx.y;
    nr_finalize_body(a, reg + s, means + s * 2 * a.nitems, scratch + s * sstride, term);
}

// ---- backward: d reg / d n0[y][x] = sum_l 4^-l (2 mx_l / cnt_l (W + E) + 2 my_l / cnt_l (N + S)) of the ancestor ----
__device__ __forceinline__ void nr_bwd_body(const NrArgs& a, int blk, int64_t samp, float* __restrict__ gflat,
                                            const float* __restrict__ greg, const float* __restrict__ means,
                                            const float* __restrict__ flat, const float* __restrict__ scratch,
                                            int accumulate) {
    const int b = nr_find(a.bwd_blk, a.nbuf, blk);
    const int c = blk - a.bwd_blk[b];
    const int R = a.R[b], nlev = a.nlev[b];
    const int e = c * NR_CHUNK + (int)threadIdx.x * 4;
    if (e >= R * R) return;
    const int y = e / R, x = e - y * R;
    const float g = greg[0];
    const float2* mean = (const float2*)(means + 2 * a.item0[b]);
    float acc[4];
    {
        const int m = R - 1;
        const float* p = flat + a.off[b] + samp * R * R;
        const float2 mm = mean[0];
        const float cnt = (float)(R * R);
        const float cx = 2.f * mm.x / cnt, cy = 2.f * mm.y / cnt;
        const float4 o = *(const float4*)(p + e);
        const float4 up = *(const float4*)(p + ((y - 1) & m) * R + x);
        const float4 dn = *(const float4*)(p + ((y + 1) & m) * R + x);
        const float lf = p[y * R + ((x - 1) & m)], rt = p[y * R + ((x + 4) & m)];
        acc[0] = cx * (lf + o.y) + cy * (up.x + dn.x);
        acc[1] = cx * (o.x + o.z) + cy * (up.y + dn.y);
        acc[2] = cx * (o.y + o.w) + cy * (up.z + dn.z);
        acc[3] = cx * (o.z + rt) + cy * (up.w + dn.w);
    }
    const float* pool = scratch + a.soff[b];
    float w = 1.f;
    for (int l = 1; l < nlev; ++l) {
        const int S = R >> l, m = S - 1;
        const float* p = pool + nr_level_off(R, l);
        const float2 mm = mean[l];
        const float cnt = (float)(S * S);
        w *= 0.25f;
        const float cx = 2.f * mm.x / cnt * w, cy = 2.f * mm.y / cnt * w;
        const int ay = y >> l;
        const int na = l == 1 ? 2 : 1;                  // the four elements have two ancestors at level 1, else one
        for (int q = 0; q < na; ++q) {
            const int ax = (x + 2 * q) >> l;
            const float v = cx * (p[ay * S + ((ax - 1) & m)] + p[ay * S + ((ax + 1) & m)]) +
                            cy * (p[((ay - 1) & m) * S + ax] + p[((ay + 1) & m) * S + ax]);
            if (na == 2) { acc[2 * q] += v; acc[2 * q + 1] += v; }
            else { acc[0] += v; acc[1] += v; acc[2] += v; acc[3] += v; }
        }
    }
    float4* out = (float4*)(gflat + a.off[b] + samp * R * R + e);
    float4 r = float4{acc[0] * g, acc[1] * g, acc[2] * g, acc[3] * g};
    if (accumulate) {
        const float4 old = *out;
        r.x += old.x; r.y += old.y; r.z += old.z; r.w += old.w;
    }
    *out = r;
}

__global__ __launch_bounds__(256) void nr_bwd_kernel(NrArgs a, float* __restrict__ gflat, const float* __restrict__ greg,
                                                     const float* __restrict__ means, const float* __restrict__ flat,
                                                     const float* __restrict__ scratch, int accumulate) {
    nr_bwd_body(a, blockIdx.x, 0, gflat, greg, means, flat, scratch, accumulate);
}

// grid (level-0 chunks, B): sample s reads greg[s], means[s] and its own pooled levels
__global__ __launch_bounds__(256) void nr_bwd_batched_kernel(NrArgs a, float* __restrict__ gflat,
                                                             const float* __restrict__ greg,
                                                             const float* __restrict__ means,
                                                             const float* __restrict__ flat,
                                                             const float* __restrict__ scratch, int64_t sstride,
                                                             int accumulate) {
    const int64_t s = blockIdx.y;
    nr_bwd_body(a, blockIdx.x, s, gflat, greg + s, means + s * 2 * a.nitems, flat, scratch + s * sstride, accumulate);
}

// ---- normalize: a workgroup per buffer; each pass sums float4 groups of 16 per lane, then the groups ----
template <int MODE>     // 0: sum x, 1: sum (x - mu)^2
__device__ __forceinline__ float nr_grouped_sum(const float4* p, int n4, float mu) {
    float tot = 0.f;
    float4 acc = float4{0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (int i = threadIdx.x; i < n4; i += 1024) {
        float4 q = p[i];
        if (MODE == 1) {
            q.x -= mu; q.y -= mu; q.z -= mu; q.w -= mu;
            q.x *= q.x; q.y *= q.y; q.z *= q.z; q.w *= q.w;
        }
        acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
        if (++k == 16) {
            tot += (acc.x + acc.y) + (acc.z + acc.w);
            acc = float4{0.f, 0.f, 0.f, 0.f};
            k = 0;
        }
    }
    return tot + ((acc.x + acc.y) + (acc.z + acc.w));
}

__device__ __forceinline__ void nr_normalize_body(const NrArgs& a, int b, int64_t samp, float* __restrict__ flat,
                                                  float* red) {
    const int n = a.R[b] * a.R[b], n4 = n / 4;
    float4* p = (float4*)(flat + a.off[b] + samp * n);
    const float mu = block_sum<16>(nr_grouped_sum<0>(p, n4, 0.f), red) / (float)n;
    const float m2 = block_sum<16>(nr_grouped_sum<1>(p, n4, mu), red) / (float)n;
    const float rs = 1.f / sqrtf(m2);
    for (int i = threadIdx.x; i < n4; i += 1024) {
        float4 q = p[i];
        q.x = (q.x - mu) * rs; q.y = (q.y - mu) * rs; q.z = (q.z - mu) * rs; q.w = (q.w - mu) * rs;
        p[i] = q;
    }
}

__global__ __launch_bounds__(1024) void nr_normalize_kernel(NrArgs a, float* __restrict__ flat) {
    __shared__ float red[16];
    nr_normalize_body(a, blockIdx.x, 0, flat, red);
}

__global__ __launch_bounds__(1024) void nr_normalize_batched_kernel(NrArgs a, float* __restrict__ flat) {   // grid (nbuf, B)
    __shared__ float red[16];
    nr_normalize_body(a, blockIdx.x, blockIdx.y, flat, red);
}

// ---- host side ----
// table: HOST int64 [nbuf][2] = (offset of the buffer in flat, in floats; R).  Fills the kernels' argument block.
// B: samples per buffer (the batched entry points; a row's buffer then spans B R^2 floats from its offset).
int nr_plan(NrArgs& a, const char* what, const int64_t* table, int nbuf, int B = 1) {
    const std::string w(what);
    SG2_CHECK(B >= 1 && B <= NR_MAXBATCH, w + ": B must be in 1..64");
    SG2_CHECK(table, w + ": table must be non-null");
    SG2_CHECK(nbuf >= 1 && nbuf <= NR_MAXBUF, w + ": nbuf must be in 1..32");
    a = NrArgs{};
    a.nbuf = nbuf;
    int64_t so = 0;
    bool big = false;
    for (int b = 0; b < nbuf; ++b) {
        const int64_t off = table[2 * b], R = table[2 * b + 1];
        SG2_CHECK(R >= 4 && R <= 1024 && (R & (R - 1)) == 0,
                  w + ": R must be a power of two in 4..1024 (square buffers only)");
        SG2_CHECK(off >= 0 && off % 4 == 0, w + ": buffer offsets must be non-negative multiples of 4 floats");
        SG2_CHECK(off + B * R * R <= 0x7fffffffLL / 4, w + ": the flat buffer must stay below 2 GiB");
        a.R[b] = (int)R;
        a.nlev[b] = nr_levels((int)R);
        a.off[b] = off;
        a.soff[b] = so;
        so += nr_level_off((int)R, a.nlev[b]);
        big = big || R > 512;
    }
    const int tile = big ? 128 : 64;
    for (int b = 0; b < nbuf; ++b) {
        const int R = a.R[b], t = R > tile ? R / tile : 1;
        int chunks = 0;
        for (int l = 0; l < a.nlev[b]; ++l) chunks += nr_chunks(R >> l);
        a.item0[b + 1] = a.item0[b] + a.nlev[b];
        a.pool_blk[b + 1] = a.pool_blk[b] + (a.nlev[b] > 1 ? t * t : 0);
        a.corr_blk[b + 1] = a.corr_blk[b] + chunks;
        a.bwd_blk[b + 1] = a.bwd_blk[b] + nr_chunks(R);
    }
    a.nitems = a.item0[nbuf];
    a.part_off = so;                                    // a multiple of 64 floats
    return big ? 8 : 4;                                 // the pool kernel's patch
}

int64_t nr_scratch_floats(const NrArgs& a) { return a.part_off + 2 * (int64_t)a.corr_blk[a.nbuf]; }
// a sample's share of the batched scratch: the batch-1 scratch, rounded up so every share stays 16-byte aligned
int64_t nr_sample_stride(const NrArgs& a) { return (nr_scratch_floats(a) + 3) / 4 * 4; }

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_noise_reg_scratch_bytes(int64_t* bytes, const int64_t* table, int nbuf) {
    SG2_CHECK(bytes, "sg2_noise_reg_scratch_bytes: bytes must be non-null");
    NrArgs a;
    if (nr_plan(a, "sg2_noise_reg_scratch_bytes", table, nbuf) < 0) return -1;
    *bytes = nr_scratch_floats(a) * 4;
    return 0;
}

extern "C" int sg2_noise_reg_fwd(float* reg, float* means, const float* flat, const int64_t* table, int nbuf,
                                 void* scratch, void* stream) {
    NrArgs a;
    const int patch = nr_plan(a, "sg2_noise_reg_fwd", table, nbuf);
    if (patch < 0) return -1;
    SG2_CHECK(reg && means && flat && scratch, "sg2_noise_reg_fwd: reg, means, flat and scratch must be non-null");
    SG2_CHECK(((uintptr_t)flat % 16) == 0 && ((uintptr_t)scratch % 16) == 0 && ((uintptr_t)means % 8) == 0,
              "sg2_noise_reg_fwd: flat and scratch must be 16-byte aligned, means 8-byte aligned");
    hipStream_t s = as_stream(stream);
    float* sc = (float*)scratch;
    if (a.pool_blk[nbuf] > 0) {
        if (patch == 8) nr_pool_kernel<8><<<a.pool_blk[nbuf], 256, 0, s>>>(a, flat, sc);
        else nr_pool_kernel<4><<<a.pool_blk[nbuf], 256, 0, s>>>(a, flat, sc);
    }
    nr_corr_kernel<<<a.corr_blk[nbuf], 256, 0, s>>>(a, flat, sc);
    nr_finalize_kernel<<<1, 1024, 0, s>>>(a, reg, means, sc);
    return launch_status("sg2_noise_reg_fwd");
}

extern "C" int sg2_noise_reg_bwd(float* gflat, const float* greg, const float* means, const float* flat,
                                 const int64_t* table, int nbuf, const void* scratch, int accumulate, void* stream) {
    NrArgs a;
    if (nr_plan(a, "sg2_noise_reg_bwd", table, nbuf) < 0) return -1;
    SG2_CHECK(gflat && greg && means && flat && scratch,
              "sg2_noise_reg_bwd: gflat, greg, means, flat and scratch must be non-null");
    SG2_CHECK(((uintptr_t)gflat % 16) == 0 && ((uintptr_t)flat % 16) == 0 && ((uintptr_t)scratch % 16) == 0 &&
                  ((uintptr_t)means % 8) == 0,
              "sg2_noise_reg_bwd: gflat, flat and scratch must be 16-byte aligned, means 8-byte aligned");
    nr_bwd_kernel<<<a.bwd_blk[nbuf], 256, 0, as_stream(stream)>>>(a, gflat, greg, means, flat, (const float*)scratch,
                                                                 accumulate);
    return launch_status("sg2_noise_reg_bwd");
}

extern "C" int sg2_noise_normalize_multi(float* flat, const int64_t* table, int nbuf, void* stream) {
    NrArgs a;
    if (nr_plan(a, "sg2_noise_normalize_multi", table, nbuf) < 0) return -1;
    SG2_CHECK(flat, "sg2_noise_normalize_multi: flat must be non-null");
    SG2_CHECK(((uintptr_t)flat % 16) == 0, "sg2_noise_normalize_multi: flat must be 16-byte aligned");
    nr_normalize_kernel<<<nbuf, 1024, 0, as_stream(stream)>>>(a, flat);
    return launch_status("sg2_noise_normalize_multi");
}

// ---- the batched entry points: B samples per buffer, the sample a grid dimension; per sample the batch-1 code ----
extern "C" int sg2_noise_reg_batched_scratch_bytes(int64_t* bytes, const int64_t* table, int nbuf, int B) {
    SG2_CHECK(bytes, "sg2_noise_reg_batched_scratch_bytes: bytes must be non-null");
    NrArgs a;
    if (nr_plan(a, "sg2_noise_reg_batched_scratch_bytes", table, nbuf, B) < 0) return -1;
    *bytes = nr_sample_stride(a) * B * 4;
    return 0;
}

extern "C" int sg2_noise_reg_fwd_batched(float* reg, float* means, const float* flat, const int64_t* table, int nbuf,
                                         int B, void* scratch, void* stream) {
    NrArgs a;
    const int patch = nr_plan(a, "sg2_noise_reg_fwd_batched", table, nbuf, B);
    if (patch < 0) return -1;
    SG2_CHECK(reg && means && flat && scratch,
              "sg2_noise_reg_fwd_batched: reg, means, flat and scratch must be non-null");
    SG2_CHECK(((uintptr_t)flat % 16) == 0 && ((uintptr_t)scratch % 16) == 0 && ((uintptr_t)means % 8) == 0,
              "sg2_noise_reg_fwd_batched: flat and scratch must be 16-byte aligned, means 8-byte aligned");
    hipStream_t s = as_stream(stream);
    float* sc = (float*)scratch;
    const int64_t ss = nr_sample_stride(a);
    if (a.pool_blk[nbuf] > 0) {
        const dim3 grid(a.pool_blk[nbuf], B);
        if (patch == 8) nr_pool_batched_kernel<8><<<grid, 256, 0, s>>>(a, flat, sc, ss);
        else nr_pool_batched_kernel<4><<<grid, 256, 0, s>>>(a, flat, sc, ss);
    }
    nr_corr_batched_kernel<<<dim3(a.corr_blk[nbuf], B), 256, 0, s>>>(a, flat, sc, ss);
    nr_finalize_batched_kernel<<<dim3(1, B), 1024, 0, s>>>(a, reg, means, sc, ss);
    return launch_status("sg2_noise_reg_fwd_batched");
}

extern "C" int sg2_noise_reg_bwd_batched(float* gflat, const float* greg, const float* means, const float* flat,
                                         const int64_t* table, int nbuf, int B, const void* scratch, int accumulate,
                                         void* stream) {
    NrArgs a;
    if (nr_plan(a, "sg2_noise_reg_bwd_batched", table, nbuf, B) < 0) return -1;
    SG2_CHECK(gflat && greg && means && flat && scratch,
              "sg2_noise_reg_bwd_batched: gflat, greg, means, flat and scratch must be non-null");
    SG2_CHECK(((uintptr_t)gflat % 16) == 0 && ((uintptr_t)flat % 16) == 0 && ((uintptr_t)scratch % 16) == 0 &&
                  ((uintptr_t)means % 8) == 0,
              "sg2_noise_reg_bwd_batched: gflat, flat and scratch must be 16-byte aligned, means 8-byte aligned");
    nr_bwd_batched_kernel<<<dim3(a.bwd_blk[nbuf], B), 256, 0, as_stream(stream)>>>(
        a, gflat, greg, means, flat, (const float*)scratch, nr_sample_stride(a), accumulate);
    return launch_status("sg2_noise_reg_bwd_batched");
}

extern "C" int sg2_noise_normalize_batched(float* flat, const int64_t* table, int nbuf, int B, void* stream) {
    NrArgs a;
    if (nr_plan(a, "sg2_noise_normalize_batched", table, nbuf, B) < 0) return -1;
    SG2_CHECK(flat, "sg2_noise_normalize_batched: flat must be non-null");
    SG2_CHECK(((uintptr_t)flat % 16) == 0, "sg2_noise_normalize_batched: flat must be 16-byte aligned");
    nr_normalize_batched_kernel<<<dim3(nbuf, B), 1024, 0, as_stream(stream)>>>(a, flat);
    return launch_status("sg2_noise_normalize_batched");
}
