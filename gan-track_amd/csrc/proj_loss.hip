// The per-sample loss of a batched latent projection step (genlib/projector/projector.py forward_batch): what the
// reference composes per projection from ~15 elementwise and reduction launches per modality, here for B projections
// at once with PER-SAMPLE results.  Latency-bound: what counts is the launch count and fixed trees, not bandwidth.
//
//   sg2_proj_prep_fwd (2 launches): synth [B, C, H, W] (the generator's output), target [B, C, H, W] in [0, 255] ->
//       det_in [M B, 3, Hd, Wd]  the detector's input, row m B + b: s = (x + 1) * 127.5 (an add and a multiply, two
//                                roundings, never an FMA, as sg2_ppl_prep), above 256^2 the mean of s over f x f
//                                (f = H / 256), channels by projector.split_modalities' rule;
//       pix [B][M]               mean (t - s)^2 over the modality's channels at full resolution.
//   sg2_proj_prep_bwd (1 launch): gsynth, every element assigned once.
//   sg2_sqdist_rows_fwd (2 launches): dist[r] = sum_j (f[r][j] - tf[r][j])^2 on sg2_lpips_pair_dist's tree
//       (sqdist_tree.h), two row pointers, no concatenated copy;  sg2_sqdist_rows_bwd (1 launch): gf = 2 g[r] (f - tf).
//
// Channel rule: C = 1: one modality, its channel repeated to three; C = 3: one RGB modality as it is; any other C: C
// modalities, each channel repeated.  A repeated modality's three channels are equal, in s and in t alike, so its mean
// over 3 H W terms is the mean over its H W source elements; n_m = the modality's source elements (H W, or 3 H W for
// RGB).
//
// pix, the summation tree (it depends on C and H only -- not on B, the sample or any address):
//   a modality's source elements are cut into groups: group g = (source channel, output row oy, four output columns)
//   holds f rows of 4 f elements; workgroup c of 256 threads takes groups 256 c .. 256 c + 255;
//   stage 1: a thread keeps four accumulators, one per output column, each a SERIAL RUN of the f^2 squares under that
//     column (rows outer, columns inner; f <= 4: 16 terms); the four are added as a tree of depth 2, then a wave
//     butterfly (6), then the four waves (2);
//   stage 2 (one workgroup per (b, m)): thread t adds the partials t, t + 256, ... (at most 192 partials: one term),
//     butterfly (6), waves (2), one division by n_m.
// No atomics.
#include "sqdist_tree.h"

namespace sg2 {
namespace {

struct ProjArgs {
    int B, C, H, M, nsrc;           // M modalities of nsrc source channels each (1, or 3 for RGB)
    int f, Hd, groups_row;          // the pooling factor, the detector's side, Hd / 4
    int groups;                     // groups of a modality: nsrc * Hd * groups_row
    int chunks;                     // workgroups of a modality: ceil(groups / 256)
    float inv;                      // 1 / f^2 (exact: f is a power of two)
    float n_m;                      // nsrc * H * H (< 2^24: exact)
};

__device__ __forceinline__ float proj_scale(float x) {      // two roundings, never an FMA
    return __fmul_rn(__fadd_rn(x, 1.f), 127.5f);
}

template <int FAC>      // 1, 2, 4
__global__ __launch_bounds__(256) void proj_prep_kernel(ProjArgs a, float* __restrict__ det_in, float* __restrict__ part,
                                                        const float* __restrict__ synth,
                                                        const float* __restrict__ target) {
    __shared__ float red[4];
    const int row = blockIdx.y, m = row / a.B, b = row - m * a.B;       // det_in's row m B + b
    const int g = blockIdx.x * 256 + threadIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (g < a.groups) {
        const int gx = g % a.groups_row, oy = (g / a.groups_row) % a.Hd, s = g / (a.groups_row * a.Hd);
        const int c = a.nsrc == 3 ? s : m;                              // the source channel (C = 1: m = 0)
        const int64_t base = ((int64_t)b * a.C + c) * a.H * a.H + (int64_t)(oy * FAC) * a.H + gx * 4 * FAC;
        float mean[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int fy = 0; fy < FAC; ++fy) {
#pragma unroll
            for (int k = 0; k < FAC; ++k) {                             // float4 k: inputs 4 k .. 4 k + 3 of the 4 FAC
                const float4 x = *(const float4*)(synth + base + (int64_t)fy * a.H + 4 * k);
                const float4 t = *(const float4*)(target + base + (int64_t)fy * a.H + 4 * k);
                const float xs[4] = {x.x, x.y, x.z, x.w}, ts[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float sv = proj_scale(xs[i]);
                    const int o = (4 * k + i) / FAC;                    // the output column this input lies under
                    mean[o] = FAC == 1 ? sv : __fadd_rn(mean[o], sv);
                    acc[o] = __fadd_rn(acc[o], ppl_sq(ts[i], sv));
                }
            }
        }
        float4 r;
        r.x = FAC == 1 ? mean[0] : __fmul_rn(mean[0], a.inv);
        r.y = FAC == 1 ? mean[1] : __fmul_rn(mean[1], a.inv);
        r.z = FAC == 1 ? mean[2] : __fmul_rn(mean[2], a.inv);
        r.w = FAC == 1 ? mean[3] : __fmul_rn(mean[3], a.inv);
        const int64_t plane = (int64_t)a.Hd * a.Hd;
        const int o_lo = a.nsrc == 3 ? s : 0, o_hi = a.nsrc == 3 ? s + 1 : 3;
        for (int o = o_lo; o < o_hi; ++o)
            *(float4*)(det_in + ((int64_t)row * 3 + o) * plane + (int64_t)oy * a.Hd + gx * 4) = r;
    }
    const float v = ppl_block_sum(__fadd_rn(__fadd_rn(acc[0], acc[2]), __fadd_rn(acc[1], acc[3])), red);
    if (threadIdx.x == 0) part[(int64_t)row * a.chunks + blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void proj_pix_final_kernel(ProjArgs a, float* __restrict__ pix,
                                                             const float* __restrict__ part) {
    __shared__ float red[4];
    const int row = blockIdx.x, m = row / a.B, b = row - m * a.B;
    const float v = sqdist_final_sum(part + (int64_t)row * a.chunks, a.chunks, red);
    if (threadIdx.x == 0) pix[b * a.M + m] = __fdiv_rn(v, a.n_m);
}

// gsynth[b][c][y][x] = 127.5 (sum over the det_in channels that read (b, c) of gdet_in[.][y / f][x / f] / f^2
//                             + gpix[b][m] 2 (s - t) / n_m);  a thread makes four neighbouring elements.
__global__ __launch_bounds__(256) void proj_prep_bwd_kernel(ProjArgs a, float* __restrict__ gsynth,
                                                            const float* __restrict__ gdet_in,
                                                            const float* __restrict__ gpix,
                                                            const float* __restrict__ synth,
                                                            const float* __restrict__ target, int64_t total4) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const int w4 = a.H / 4;
    const int x0 = (int)(idx % w4) * 4, y = (int)((idx / w4) % a.H);
    const int c = (int)((idx / ((int64_t)w4 * a.H)) % a.C), b = (int)(idx / ((int64_t)w4 * a.H * a.C));
    const int m = a.nsrc == 3 ? 0 : c;                                  // (C = 1: c = 0)
    const int row = m * a.B + b;
    const int64_t e = idx * 4, plane = (int64_t)a.Hd * a.Hd;
    const float4 x = *(const float4*)(synth + e), t = *(const float4*)(target + e);
    const float xs[4] = {x.x, x.y, x.z, x.w}, ts[4] = {t.x, t.y, t.z, t.w};
    const float gp = 2.f * gpix[b * a.M + m] / a.n_m;
    const float* gd = gdet_in + (int64_t)row * 3 * plane + (int64_t)(y / a.f) * a.Hd;
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ox = (x0 + i) / a.f;
        const float gdet = a.nsrc == 3 ? gd[c * plane + ox] : (gd[ox] + gd[plane + ox]) + gd[2 * plane + ox];
        r[i] = 127.5f * (gdet * a.inv + gp * (proj_scale(xs[i]) - ts[i]));
    }
    *(float4*)(gsynth + e) = make_float4(r[0], r[1], r[2], r[3]);
}

int proj_plan(ProjArgs& a, const char* what, int B, int C, int H) {
    const std::string w(what);
    SG2_CHECK(B >= 1 && B <= 4096, w + ": B must be in 1..4096");
    SG2_CHECK(C >= 1 && C <= 16, w + ": C must be in 1..16");
    SG2_CHECK(H >= 4 && H <= 1024 && (H & (H - 1)) == 0, w + ": H must be a power of two in 4..1024 (square images)");
    a = ProjArgs{};
    a.B = B; a.C = C; a.H = H;
    a.nsrc = C == 3 ? 3 : 1;
    a.M = (C == 1 || C == 3) ? 1 : C;
    a.f = H > 256 ? H / 256 : 1;
    a.Hd = H / a.f;
    a.groups_row = a.Hd / 4;
    a.groups = a.nsrc * a.Hd * a.groups_row;
    a.chunks = (a.groups + 255) / 256;
    a.inv = 1.f / (float)(a.f * a.f);
    a.n_m = (float)a.nsrc * (float)H * (float)H;
    return 0;
}

template <bool VEC>
__global__ __launch_bounds__(PPL_THREADS) void sqdist_rows_partial_kernel(const float* __restrict__ f,
                                                                          const float* __restrict__ tf, int64_t F,
                                                                          int64_t chunks, float* __restrict__ part) {
    __shared__ float red[4];
    const int64_t r = blockIdx.y, c = blockIdx.x;
    const float v = sqdist_chunk_sum<VEC>(f + r * F, tf + r * F, F, c, red);
    if (threadIdx.x == 0) part[r * chunks + c] = v;
}

__global__ __launch_bounds__(PPL_THREADS) void sqdist_rows_final_kernel(const float* __restrict__ part, int64_t chunks,
                                                                        float* __restrict__ dist) {
    __shared__ float red[4];
    const float v = sqdist_final_sum(part + (int64_t)blockIdx.x * chunks, chunks, red);
    if (threadIdx.x == 0) dist[blockIdx.x] = v;
}

template <bool VEC>     // grid (ceil(F / 1024), R): a thread makes four neighbouring elements of a row
__global__ __launch_bounds__(256) void sqdist_rows_bwd_kernel(float* __restrict__ gf, const float* __restrict__ g,
                                                              const float* __restrict__ f, const float* __restrict__ tf,
                                                              int64_t F) {
    const int64_t r = blockIdx.y, j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (j >= F) return;
    const float s = 2.f * g[r];
    const int64_t e = r * F + j;
    if (VEC) {
        const float4 a = *(const float4*)(f + e), b = *(const float4*)(tf + e);
        *(float4*)(gf + e) = make_float4(s * (a.x - b.x), s * (a.y - b.y), s * (a.z - b.z), s * (a.w - b.w));
    } else {
        for (int i = 0; i < 4 && j + i < F; ++i) gf[e + i] = s * (f[e + i] - tf[e + i]);
    }
}

int sqdist_plan(const char* what, int64_t R, int64_t F, int64_t& chunks) {
    const std::string w(what);
    SG2_CHECK(R >= 1 && R <= 65535, w + ": R must be in 1..65535");
    SG2_CHECK(F >= 1 && F <= (int64_t)1 << 40, w + ": F must be in 1..2^40");
    chunks = cdiv(F, PPL_CHUNK);
    SG2_CHECK(chunks <= 0x7fffffffLL / 8, w + ": F is too large for one launch");
    return 0;
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_proj_prep_scratch_bytes(int64_t* bytes, int B, int C, int H) {
    SG2_CHECK(bytes, "sg2_proj_prep_scratch_bytes: bytes must be non-null");
    ProjArgs a;
    if (proj_plan(a, "sg2_proj_prep_scratch_bytes", B, C, H) < 0) return -1;
    *bytes = (int64_t)a.M * B * a.chunks * 4;
    return 0;
}

extern "C" int sg2_proj_prep_fwd(float* det_in, float* pix, const float* synth, const float* target, int B, int C, int H,
                                 void* scratch, int64_t scratch_bytes, void* stream) {
    ProjArgs a;
    if (proj_plan(a, "sg2_proj_prep_fwd", B, C, H) < 0) return -1;
    SG2_CHECK(det_in && pix && synth && target && scratch,
              "sg2_proj_prep_fwd: det_in, pix, synth, target and scratch must be non-null");
    SG2_CHECK(((uintptr_t)det_in % 16) == 0 && ((uintptr_t)synth % 16) == 0 && ((uintptr_t)target % 16) == 0 &&
                  ((uintptr_t)scratch % 4) == 0 && ((uintptr_t)pix % 4) == 0,
              "sg2_proj_prep_fwd: det_in, synth and target must be 16-byte aligned, pix and scratch 4-byte aligned");
    SG2_CHECK(scratch_bytes >= (int64_t)a.M * B * a.chunks * 4,
              "sg2_proj_prep_fwd: scratch too small (sg2_proj_prep_scratch_bytes)");
    SG2_CHECK((int64_t)a.M * B <= 65535, "sg2_proj_prep_fwd: too many (modality, sample) rows for one launch");
    hipStream_t s = as_stream(stream);
    float* part = (float*)scratch;
    const dim3 grid(a.chunks, a.M * B);
    switch (a.f) {
        case 1: proj_prep_kernel<1><<<grid, 256, 0, s>>>(a, det_in, part, synth, target); break;
        case 2: proj_prep_kernel<2><<<grid, 256, 0, s>>>(a, det_in, part, synth, target); break;
        default: proj_prep_kernel<4><<<grid, 256, 0, s>>>(a, det_in, part, synth, target); break;
    }
    proj_pix_final_kernel<<<a.M * B, 256, 0, s>>>(a, pix, part);
    return launch_status("sg2_proj_prep_fwd");
}

extern "C" int sg2_proj_prep_bwd(float* gsynth, const float* gdet_in, const float* gpix, const float* synth,
                                 const float* target, int B, int C, int H, void* stream) {
    ProjArgs a;
    if (proj_plan(a, "sg2_proj_prep_bwd", B, C, H) < 0) return -1;
    SG2_CHECK(gsynth && gdet_in && gpix && synth && target,
              "sg2_proj_prep_bwd: gsynth, gdet_in, gpix, synth and target must be non-null");
    SG2_CHECK(((uintptr_t)gsynth % 16) == 0 && ((uintptr_t)synth % 16) == 0 && ((uintptr_t)target % 16) == 0 &&
                  ((uintptr_t)gdet_in % 4) == 0 && ((uintptr_t)gpix % 4) == 0,
              "sg2_proj_prep_bwd: gsynth, synth and target must be 16-byte aligned, gdet_in and gpix 4-byte aligned");
    const int64_t total4 = (int64_t)B * C * H * H / 4;
    SG2_CHECK(cdiv(total4, 256) <= 0x7fffffffLL, "sg2_proj_prep_bwd: the image batch is too large for one launch");
    proj_prep_bwd_kernel<<<(unsigned)cdiv(total4, 256), 256, 0, as_stream(stream)>>>(a, gsynth, gdet_in, gpix, synth,
                                                                                     target, total4);
    return launch_status("sg2_proj_prep_bwd");
}

extern "C" int sg2_sqdist_rows_scratch_bytes(int64_t* bytes, int64_t R, int64_t F) {
    SG2_CHECK(bytes, "sg2_sqdist_rows_scratch_bytes: bytes must be non-null");
    int64_t chunks;
    if (sqdist_plan("sg2_sqdist_rows_scratch_bytes", R, F, chunks) < 0) return -1;
    *bytes = R * chunks * 4;
    return 0;
}

extern "C" int sg2_sqdist_rows_fwd(float* dist, const float* f, const float* tf, int64_t R, int64_t F, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
    int64_t chunks;
    if (sqdist_plan("sg2_sqdist_rows_fwd", R, F, chunks) < 0) return -1;
    SG2_CHECK(dist && f && tf && scratch, "sg2_sqdist_rows_fwd: dist, f, tf and scratch must be non-null");
    SG2_CHECK(scratch_bytes >= R * chunks * 4, "sg2_sqdist_rows_fwd: scratch too small (sg2_sqdist_rows_scratch_bytes)");
    SG2_CHECK(((uintptr_t)f % 4) == 0 && ((uintptr_t)tf % 4) == 0 && ((uintptr_t)scratch % 4) == 0 &&
                  ((uintptr_t)dist % 4) == 0,
              "sg2_sqdist_rows_fwd: dist, f, tf and scratch must be 4-byte aligned");
    hipStream_t s = as_stream(stream);
    float* part = (float*)scratch;
    const dim3 grid((unsigned)chunks, (unsigned)R);
    if (((uintptr_t)f % 16) == 0 && ((uintptr_t)tf % 16) == 0 && F % 4 == 0)
        sqdist_rows_partial_kernel<true><<<grid, PPL_THREADS, 0, s>>>(f, tf, F, chunks, part);
    else
        sqdist_rows_partial_kernel<false><<<grid, PPL_THREADS, 0, s>>>(f, tf, F, chunks, part);
    sqdist_rows_final_kernel<<<(unsigned)R, PPL_THREADS, 0, s>>>(part, chunks, dist);
    return launch_status("sg2_sqdist_rows_fwd");
}

extern "C" int sg2_sqdist_rows_bwd(float* gf, const float* g, const float* f, const float* tf, int64_t R, int64_t F,
                                   void* stream) {
    int64_t chunks;
    if (sqdist_plan("sg2_sqdist_rows_bwd", R, F, chunks) < 0) return -1;
    SG2_CHECK(gf && g && f && tf, "sg2_sqdist_rows_bwd: gf, g, f and tf must be non-null");
    SG2_CHECK(((uintptr_t)gf % 4) == 0 && ((uintptr_t)g % 4) == 0 && ((uintptr_t)f % 4) == 0 && ((uintptr_t)tf % 4) == 0,
              "sg2_sqdist_rows_bwd: gf, g, f and tf must be 4-byte aligned");
    const dim3 grid((unsigned)cdiv(F, 1024), (unsigned)R);
    hipStream_t s = as_stream(stream);
    if (((uintptr_t)gf % 16) == 0 && ((uintptr_t)f % 16) == 0 && ((uintptr_t)tf % 16) == 0 && F % 4 == 0)
        sqdist_rows_bwd_kernel<true><<<grid, 256, 0, s>>>(gf, g, f, tf, F);
    else
        sqdist_rows_bwd_kernel<false><<<grid, 256, 0, s>>>(gf, g, f, tf, F);
    return launch_status("sg2_sqdist_rows_bwd");
}
