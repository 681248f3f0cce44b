// sg2_image_tiles_u8: the generator's output stage in ONE pass -- img [N, C, H, W] (f32 / f16 / bf16) -> uint8 tiles of
// an HWC canvas [gh * H, gw * W, Cout].  The reference composes it from mul, add, clamp, cast (or sub, mul, rint,
// clip, cast on the host) plus a permute / reshape layout pass (SG3/gen_video.py layout_grid, gen_images*.py,
// save_image_grid): 5-7 elementwise launches per batch and four bytes per pixel over PCIe where one does.
//
// Value (include/sg2hip.h has the contract):
//   trunc: v = x * 127.5f, rounded; v + 128.0f, rounded -- two roundings, never an FMA; clamp to [0, 255]; truncate.
//   rint:  v = (x - lo) * scale with lo, scale f32 -- a subtract and a multiply, never x * scale - lo * scale;
//          round half to even; clip to [0, 255].
//   NaN -> 0, +inf -> 255, -inf -> 0 in both modes (fmaxf(NaN, 0) is 0).
// 16-bit inputs are widened to f32 first (exact).
//
// Work: one read of img, one write of the canvas, no scratch, no atomics.  Bytes outside the addressed tiles are never
// written (no read-modify-write of the canvas either).
//   wide path   Cout = 1, W % 16 == 0, img and canvas 16-byte aligned: a lane converts 16 neighbouring pixels of one
//               tile row -- 4 (f32) or 2 (16-bit) 16-byte loads, one 16-byte store.  Every row start is then 16-byte
//               aligned on both sides (row pitches and column offsets are multiples of 16 bytes).
//   dword path  anything else (W % 16 != 0, an odd canvas base, Cout = 3 where a 16-byte store would span 5 1/3 pixels):
//               a lane owns one 4-byte-ALIGNED dword of a tile row's destination bytes, whatever the row's own
//               alignment, and stores it whole; the (at most two) partial dwords at a row's ends go byte by byte.
// All offsets are 64-bit.
#include "sg2_common.h"

namespace sg2 {
namespace {

constexpr int IMG_THREADS = 256;

struct TileArgs {
    const void* img;
    uint8_t* canvas;
    int N, C, H, W;
    int tiles;          // SG2_TILES_HWC, SG2_TILES_GREY, or a channel >= 0
    int gw;
    int64_t first_tile;
    float lo, scale;    // rint mode
    int64_t total;      // lanes with work
    int per_row;        // lanes per tile row
};

template <bool RINT>
__device__ __forceinline__ unsigned to_u8(float x, float lo, float scale) {
    // hipcc contracts by default, and HIP's __fmul_rn / __fadd_rn are a plain * and + that it contracts all the same:
    // x * 127.5f + 128.0f became one v_fma (95 of the 768 boundary values of the tests change their byte).
#pragma clang fp contract(off)
    float v;
    if (RINT) {
        v = rintf((x - lo) * scale);
    } else {
        const float m = x * 127.5f;
        v = m + 128.0f;
    }
    v = fminf(fmaxf(v, 0.f), 255.f);    // NaN -> 0
    return (unsigned)(int)v;
}

// tile t -> image n and (for Cout = 1) source channel c
template <typename IDX>
__device__ __forceinline__ void tile_source(const TileArgs& a, IDX t, int64_t& n, int& c) {
    if (a.tiles == SG2_TILES_GREY) { n = (int64_t)(t / (IDX)a.C); c = (int)(t % (IDX)a.C); }
    else { n = (int64_t)t; c = a.tiles >= 0 ? a.tiles : 0; }
}

template <typename T, bool RINT, typename IDX>
__global__ __launch_bounds__(IMG_THREADS) void tiles_wide_kernel(TileArgs a) {
    const int64_t idx64 = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x;
    if (idx64 >= a.total) return;
    const IDX idx = (IDX)idx64;
    const int g = (int)(idx % (IDX)a.per_row);
    const IDX line = idx / (IDX)a.per_row;
    const int y = (int)(line % (IDX)a.H);
    const IDX t = line / (IDX)a.H;
    int64_t n; int c;
    tile_source<IDX>(a, t, n, c);
    const IDX cell = (IDX)a.first_tile + t;
    const int64_t row = (int64_t)(cell / (IDX)a.gw), col = (int64_t)(cell % (IDX)a.gw);
    const T* src = (const T*)a.img + ((n * a.C + c) * a.H + y) * a.W + g * 16;
    uint8_t* dst = a.canvas + (row * a.H + y) * ((int64_t)a.gw * a.W) + col * a.W + g * 16;
    float x[16];
    if (sizeof(T) == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 q = ((const float4*)src)[k];
            x[4 * k] = q.x; x[4 * k + 1] = q.y; x[4 * k + 2] = q.z; x[4 * k + 3] = q.w;
        }
    } else {
        typedef T vec8 __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const vec8 q = ((const vec8*)src)[k];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[8 * k + i] = (float)q[i];
        }
    }
    uint4 o;
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = to_u8<RINT>(x[4 * k], a.lo, a.scale) | (to_u8<RINT>(x[4 * k + 1], a.lo, a.scale) << 8) |
               (to_u8<RINT>(x[4 * k + 2], a.lo, a.scale) << 16) | (to_u8<RINT>(x[4 * k + 3], a.lo, a.scale) << 24);
    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    *(uint4*)dst = o;
}

// COUT = 1: a tile is one plane; COUT = 3: destination byte j of a row is channel j % 3 of pixel j / 3.
template <typename T, bool RINT, int COUT, typename IDX>
__global__ __launch_bounds__(IMG_THREADS) void tiles_dword_kernel(TileArgs a) {
    const int64_t idx64 = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x;
    if (idx64 >= a.total) return;
    const IDX idx = (IDX)idx64;
    const int g = (int)(idx % (IDX)a.per_row);
    const IDX line = idx / (IDX)a.per_row;
    const int y = (int)(line % (IDX)a.H);
    const IDX t = line / (IDX)a.H;
    int64_t n; int c;
    tile_source<IDX>(a, t, n, c);
    const IDX cell = (IDX)a.first_tile + t;
    const int64_t row = (int64_t)(cell / (IDX)a.gw), col = (int64_t)(cell % (IDX)a.gw);
    const int64_t plane = (int64_t)a.H * a.W;
    const T* src = (const T*)a.img + (n * a.C + c) * plane + (int64_t)y * a.W;     // channel c (COUT = 3: c = 0) row y
    const int rb = a.W * COUT;                                                      // the row's destination bytes
    uint8_t* dst = a.canvas + ((row * a.H + y) * ((int64_t)a.gw * a.W) + col * a.W) * COUT;
    // lane g owns the aligned dword g of those that overlap [dst, dst + rb): row bytes j0 .. j0 + 3, j0 in -3 ..
    const int j0 = g * 4 - (int)((uintptr_t)dst & 3);
    if (j0 >= rb) return;
    unsigned b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = j0 + i;
        b[i] = 0;
        if (j >= 0 && j < rb) {
            const T v = COUT == 1 ? src[j] : src[(int64_t)(j % COUT) * plane + j / COUT];
            b[i] = to_u8<RINT>((float)v, a.lo, a.scale);
        }
    }
    if (j0 >= 0 && j0 + 4 <= rb) {
        *(unsigned*)(dst + j0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j0 + i >= 0 && j0 + i < rb) dst[j0 + i] = (uint8_t)b[i];
    }
}

// IDX: the type the lane number and the grid cell are taken apart in -- 32-bit when both fit (a 64-bit division costs
// some forty instructions, three of them per lane); addresses are 64-bit either way.
template <typename T, bool RINT, typename IDX>
void launch_tiles_idx(const TileArgs& a, bool wide, int cout, unsigned blocks, hipStream_t s) {
    if (wide) tiles_wide_kernel<T, RINT, IDX><<<blocks, IMG_THREADS, 0, s>>>(a);
    else if (cout == 1) tiles_dword_kernel<T, RINT, 1, IDX><<<blocks, IMG_THREADS, 0, s>>>(a);
    else tiles_dword_kernel<T, RINT, 3, IDX><<<blocks, IMG_THREADS, 0, s>>>(a);
}
template <typename T, bool RINT>
void launch_tiles(const TileArgs& a, bool wide, int cout, bool small, unsigned blocks, hipStream_t s) {
    if (small) launch_tiles_idx<T, RINT, uint32_t>(a, wide, cout, blocks, s);
    else launch_tiles_idx<T, RINT, int64_t>(a, wide, cout, blocks, s);
}

}  // namespace
}  // namespace sg2

using namespace sg2;

extern "C" int sg2_image_tiles_u8(uint8_t* canvas, const void* img, int dtype, int N, int C, int H, int W, int tiles,
                                  int mode, double lo, double hi, int gw, int gh, int64_t first_tile, void* stream) {
    SG2_CHECK(canvas && img, "sg2_image_tiles_u8: canvas and img must be non-null");
    SG2_CHECK(dtype == SG2_F32 || dtype == SG2_F16 || dtype == SG2_BF16,
              "sg2_image_tiles_u8: dtype must be SG2_F32, SG2_F16 or SG2_BF16");
    SG2_CHECK(N >= 1 && C >= 1 && H >= 1 && W >= 1, "sg2_image_tiles_u8: N, C, H and W must be at least 1");
    SG2_CHECK(tiles == SG2_TILES_HWC || tiles == SG2_TILES_GREY || (tiles >= 0 && tiles < C),
              "sg2_image_tiles_u8: tiles must be SG2_TILES_HWC, SG2_TILES_GREY or a channel of img");
    SG2_CHECK(tiles != SG2_TILES_HWC || C == 1 || C == 3, "sg2_image_tiles_u8: tiles SG2_TILES_HWC needs C = 1 or C = 3");
    SG2_CHECK(mode == SG2_U8_TRUNC || mode == SG2_U8_RINT, "sg2_image_tiles_u8: mode must be SG2_U8_TRUNC or SG2_U8_RINT");
    SG2_CHECK(gw >= 1 && gh >= 1, "sg2_image_tiles_u8: the grid (gw, gh) must be at least 1 x 1");
    const int64_t T = tiles == SG2_TILES_GREY ? (int64_t)N * C : N;
    SG2_CHECK(first_tile >= 0 && first_tile + T <= (int64_t)gw * gh,
              "sg2_image_tiles_u8: first_tile + the number of tiles exceeds the grid gw * gh");
    float lo_f = 0.f, scale_f = 0.f;
    if (mode == SG2_U8_RINT) {
        SG2_CHECK(lo == lo && hi == hi && hi != lo && (hi - lo) * 0 == 0,
                  "sg2_image_tiles_u8: lo and hi must be finite and differ");
        lo_f = (float)lo;
        scale_f = (float)(255.0 / (hi - lo));   // formed in double, cast once
    }
    const int cout = (tiles == SG2_TILES_HWC) ? C : 1;
    const int esize = dtype == SG2_F32 ? 4 : 2;
    SG2_CHECK(((uintptr_t)img % esize) == 0, "sg2_image_tiles_u8: img must be aligned to its element size");
    SG2_CHECK((int64_t)W * cout <= 0x7fffffffLL - 8, "sg2_image_tiles_u8: a tile row is too long");
    const bool wide = cout == 1 && W % 16 == 0 && ((uintptr_t)img % 16) == 0 && ((uintptr_t)canvas % 16) == 0;
    TileArgs a;
    a.img = img; a.canvas = canvas;
    a.N = N; a.C = C; a.H = H; a.W = W;
    a.tiles = tiles; a.gw = gw; a.first_tile = first_tile;
    a.lo = lo_f; a.scale = scale_f;
    a.per_row = wide ? W / 16 : (W * cout) / 4 + 2;     // dword path: 3 bytes of lead-in at the most
    a.total = T * H * a.per_row;
    const int64_t blocks = cdiv(a.total, IMG_THREADS);
    SG2_CHECK(blocks <= 0x7fffffffLL, "sg2_image_tiles_u8: the image batch is too large for one launch");
    const bool small = a.total <= 0x7fffffffLL && (int64_t)gw * gh <= 0x7fffffffLL;
    hipStream_t s = as_stream(stream);
    if (mode == SG2_U8_RINT) {
        SG2_DISPATCH(dtype, T_, (launch_tiles<T_, true>(a, wide, cout, small, (unsigned)blocks, s)));
    } else {
        SG2_DISPATCH(dtype, T_, (launch_tiles<T_, false>(a, wide, cout, small, (unsigned)blocks, s)));
    }
    return launch_status("sg2_image_tiles_u8");
}
