// The two streaming passes of one perceptual-path-length sampler call (SG3/metrics/perceptual_path_length.py:71-89):
//   sg2_ppl_prep:          crop -> mean over factor x factor -> (x + 1) * 127.5 -> one channel repeated to three, the
//                          detector's input in ONE pass (the reference: slice, reshape + mean, add, mul, repeat);
//   sg2_lpips_pair_dist:   dist[b] = sum_j (feats[b][j] - feats[B + b][j])^2 / (float)(eps * eps) in ONE read of the
//                          features (the reference: sub, square, sum -- three passes, two temporaries of the features'
//                          size, 7,995,392 floats per image for VGG16 at 256^2).
// Both are HBM-bound: what counts is one pass and 16-byte accesses.
//
// sg2_lpips_pair_dist's summation tree (it depends on F only -- not on B, the pair's row, or any address) is
// sqdist_tree.h's, shared with sg2_sqdist_rows_fwd: serial runs of 8, then ceil(ceil(F / 8192) / 256) (4 at
// F = 7,995,392), tree depth 18 (PPL_SERIAL / PPL_DEPTH there; torch_utils/ops/ppl.py pair_dist_tree(F) restates them
// for the tests' bound).  No atomics; elements past F add +0.  Rows that are 16-byte aligned (feats aligned,
// F % 4 == 0) are read as float4, any others element by element on the SAME tree.
#include "sqdist_tree.h"

namespace sg2 {
namespace {

template <bool VEC>
__global__ __launch_bounds__(PPL_THREADS) void ppl_dist_partial_kernel(const float* __restrict__ feats, int64_t B,
                                                                       int64_t F, int64_t chunks,
                                                                       float* __restrict__ part) {
    __shared__ float red[4];
    const int64_t b = blockIdx.y, c = blockIdx.x;
    const float v = sqdist_chunk_sum<VEC>(feats + b * F, feats + (B + b) * F, F, c, red);
    if (threadIdx.x == 0) part[b * chunks + c] = v;
}

__global__ __launch_bounds__(PPL_THREADS) void ppl_dist_final_kernel(const float* __restrict__ part, int64_t chunks,
                                                                     float eps2, float* __restrict__ dist) {
    __shared__ float red[4];
    const float v = sqdist_final_sum(part + (int64_t)blockIdx.x * chunks, chunks, red);
    if (threadIdx.x == 0) dist[blockIdx.x] = __fdiv_rn(v, eps2);
}

// ---- sg2_ppl_prep: a thread makes four neighbouring outputs of one output row (the last group of a row may be
// shorter) from FAC rows of 4 * FAC inputs, for one source channel, and stores them to one or to all three output
// channels.  Inputs and outputs go as float4 where the group is whole and its address 16-byte aligned -- every group
// when W, the crop offset and Wo are multiples of 4 (256^2 and 1024^2, cropped or not) -- else element by element: a
// crop at H = 24 starts 6 floats into the row, and a 3 x 3 output plane shifts every row's and channel's alignment.
// FAC = 0: any other factor, at run time, element by element.
struct PrepArgs {
    const float* img;
    float* out;
    int N, C, H, W;
    int y0, x0, Ho, Wo, factor, groups;     // the crop window's origin; the output extent; groups = ceil(Wo / 4)
    int channel;                            // the one source channel, or -1: output channel o reads source o % C
    float inv;                              // 1 / factor^2
    int64_t total;                          // N * Ho * groups
};

template <int FAC>
__global__ __launch_bounds__(256) void ppl_prep_kernel(PrepArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const int g = (int)(idx % a.groups);
    const int oy = (int)((idx / a.groups) % a.Ho);
    const int n = (int)(idx / ((int64_t)a.groups * a.Ho));
    constexpr int FF = FAC ? FAC : 1;
    const int f = FAC ? FAC : a.factor;
    const int ox0 = g * 4, cnt = min(4, a.Wo - ox0);
    const int nsrc = (a.channel < 0 && a.C == 3) ? 3 : 1;
    const int64_t plane_in = (int64_t)a.H * a.W, plane_out = (int64_t)a.Ho * a.Wo;
    for (int s = 0; s < nsrc; ++s) {
        const int sc = a.channel >= 0 ? a.channel : s;      // (C == 1 with channel -1: source 0)
        const float* src = a.img + ((int64_t)n * a.C + sc) * plane_in + (int64_t)(a.y0 + oy * f) * a.W + a.x0 +
                           (int64_t)ox0 * f;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const bool vin = FAC && cnt == 4 && ((uintptr_t)src % 16) == 0 && (FAC == 1 || a.W % 4 == 0);
        if (FAC == 1) {
            if (vin) {
                const float4 q = *(const float4*)src;
                acc[0] = q.x; acc[1] = q.y; acc[2] = q.z; acc[3] = q.w;
            } else {
                for (int i = 0; i < cnt; ++i) acc[i] = src[i];
            }
        } else if (FAC && vin) {
#pragma unroll
            for (int fy = 0; fy < FF; ++fy) {
                const float* row = src + (int64_t)fy * a.W;
#pragma unroll
                for (int k = 0; k < FF; ++k) {     // float4 k holds inputs 4k .. 4k + 3 of the row's 4 * FAC
                    const float4 q = *(const float4*)(row + 4 * k);
                    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[(4 * k + i) / FF] += e[i];
                }
            }
        } else {
            for (int fy = 0; fy < f; ++fy) {
                const float* row = src + (int64_t)fy * a.W;
                for (int i = 0; i < cnt; ++i)
                    for (int fx = 0; fx < f; ++fx) acc[i] += row[i * f + fx];
            }
        }
        float r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {       // two roundings, never an FMA: (x + 1) * (255 / 2) as torch composes it
            const float m = FAC == 1 ? acc[i] : __fmul_rn(acc[i], a.inv);
            r[i] = __fmul_rn(__fadd_rn(m, 1.f), 127.5f);
        }
        const int o_lo = nsrc == 3 ? s : 0, o_hi = nsrc == 3 ? s + 1 : 3;
        for (int o = o_lo; o < o_hi; ++o) {
            float* dst = a.out + ((int64_t)n * 3 + o) * plane_out + (int64_t)oy * a.Wo + ox0;
            if (cnt == 4 && ((uintptr_t)dst % 16) == 0) {
                *(float4*)dst = make_float4(r[0], r[1], r[2], r[3]);
            } else {
                for (int i = 0; i < cnt; ++i) dst[i] = r[i];
            }
        }
    }
}

int pair_dist_plan(const char* what, int64_t B, int64_t F, int64_t& chunks) {
    const std::string w(what);
    SG2_CHECK(B >= 1 && B <= 65535, w + ": B must be in 1..65535");
    SG2_CHECK(F >= 1 && F <= (int64_t)1 << 40, w + ": F must be in 1..2^40");
    chunks = cdiv(F, PPL_CHUNK);
    return 0;
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_ppl_prep(float* out, const float* img, int N, int C, int H, int W, int channel, int crop, int factor,
                            void* stream) {
    SG2_CHECK(out && img, "sg2_ppl_prep: out and img must be non-null");
    SG2_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1, "sg2_ppl_prep: N, C, H and W must be at least 1");
    SG2_CHECK(crop == 0 || crop == 1, "sg2_ppl_prep: crop must be 0 or 1");
    SG2_CHECK(factor >= 1, "sg2_ppl_prep: factor must be at least 1");
    SG2_CHECK(channel >= -1 && channel < C, "sg2_ppl_prep: channel must be -1 (all) or a channel of img");
    SG2_CHECK(channel >= 0 || C == 1 || C == 3, "sg2_ppl_prep: channel -1 (all channels) needs C = 1 or C = 3");
    SG2_CHECK(!crop || (H == W && H % 8 == 0), "sg2_ppl_prep: crop needs a square image with H % 8 == 0");
    const int c8 = H / 8;
    const int Hc = crop ? 4 * c8 : H, Wc = crop ? 4 * c8 : W;
    SG2_CHECK(Hc % factor == 0 && Wc % factor == 0,
              "sg2_ppl_prep: factor must divide the (cropped) height and width");
    PrepArgs a;
    a.img = img; a.out = out;
    a.N = N; a.C = C; a.H = H; a.W = W;
    a.y0 = crop ? 3 * c8 : 0; a.x0 = crop ? 2 * c8 : 0;
    a.Ho = Hc / factor; a.Wo = Wc / factor; a.factor = factor;
    a.groups = (a.Wo + 3) / 4;
    a.channel = channel;
    a.inv = 1.f / ((float)factor * (float)factor);
    a.total = (int64_t)N * a.Ho * a.groups;
    const int64_t blocks = cdiv(a.total, 256);
    SG2_CHECK(blocks <= 0x7fffffffLL, "sg2_ppl_prep: the image batch is too large for one launch");
    hipStream_t s = as_stream(stream);
    switch (factor) {
        case 1: ppl_prep_kernel<1><<<(unsigned)blocks, 256, 0, s>>>(a); break;
        case 2: ppl_prep_kernel<2><<<(unsigned)blocks, 256, 0, s>>>(a); break;
        case 4: ppl_prep_kernel<4><<<(unsigned)blocks, 256, 0, s>>>(a); break;
        default: ppl_prep_kernel<0><<<(unsigned)blocks, 256, 0, s>>>(a); break;
    }
    return launch_status("sg2_ppl_prep");
}

extern "C" int sg2_lpips_pair_dist_scratch_bytes(int64_t* bytes, int64_t B, int64_t F) {
    SG2_CHECK(bytes, "sg2_lpips_pair_dist_scratch_bytes: bytes must be non-null");
    int64_t chunks;
    if (pair_dist_plan("sg2_lpips_pair_dist_scratch_bytes", B, F, chunks) < 0) return -1;
    *bytes = B * chunks * 4;
    return 0;
}

extern "C" int sg2_lpips_pair_dist(float* dist, const float* feats, int64_t B, int64_t F, double eps, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
    int64_t chunks;
    if (pair_dist_plan("sg2_lpips_pair_dist", B, F, chunks) < 0) return -1;
    SG2_CHECK(dist && feats && scratch, "sg2_lpips_pair_dist: dist, feats and scratch must be non-null");
    SG2_CHECK(eps > 0, "sg2_lpips_pair_dist: eps must be positive");
    SG2_CHECK(scratch_bytes >= B * chunks * 4,
              "sg2_lpips_pair_dist: scratch too small (sg2_lpips_pair_dist_scratch_bytes)");
    SG2_CHECK(((uintptr_t)feats % 4) == 0 && ((uintptr_t)scratch % 4) == 0 && ((uintptr_t)dist % 4) == 0,
              "sg2_lpips_pair_dist: dist, feats and scratch must be 4-byte aligned");
    SG2_CHECK(chunks <= 0x7fffffffLL, "sg2_lpips_pair_dist: F is too large for one launch");
    hipStream_t s = as_stream(stream);
    float* part = (float*)scratch;
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (((uintptr_t)feats % 16) == 0 && F % 4 == 0)
        ppl_dist_partial_kernel<true><<<grid, PPL_THREADS, 0, s>>>(feats, B, F, chunks, part);
    else
        ppl_dist_partial_kernel<false><<<grid, PPL_THREADS, 0, s>>>(feats, B, F, chunks, part);
    ppl_dist_final_kernel<<<(unsigned)B, PPL_THREADS, 0, s>>>(part, chunks, (float)(eps * eps), dist);
    return launch_status("sg2_lpips_pair_dist");
}
