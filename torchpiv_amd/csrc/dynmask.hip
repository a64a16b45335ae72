// Per-pair masks of moving bodies, segmented on the device from the frames themselves (defined in include/torchpiv_hip.h:
// tpiv_dynamic_mask).  Integer in, bytes 0 / 1 out, every step as tests/dynmask_model.py states it.
//
// Per frame g [H, W], odd size k = 2r + 1 in 3..63, level in 0..255, grow >= 0 with R = r + grow <= 31, every square
// neighbourhood clipped to the image:
//   core = [min over N_r of g >= level] (bright) or [max over N_r of g <= level] (dark)
//   obj  = [any core pixel in N_R];   mask of a pair = obj(a) | obj(b) | (static != 0)
// Both stencils are monotone in the threshold, so the frame is binarised as it is staged -- t = 0xFF where g >= level (g <=
// level), 0x00 elsewhere -- and what runs is the sliding minimum of prefilter.hip on those bytes, twice:
//   erode kernel:  e = min over N_r of t, pixels outside the image staged as 0xFF (a clipped neighbourhood ignores them);
//                  frame a, then frame b of the pair through the same LDS; core = e(a) | e(b) goes to the workspace, one
//                  byte (0x00 / 0xFF) per pixel and pair.  A dilation distributes over the OR, so one dilation serves both.
//   dilate kernel: d = min over N_R of ~core, outside the image again 0xFF (= no core there); mask = (d == 0) | (static != 0).
// Tile, halo, alignment and the doubling steps are prefilter.hip's: 256 lanes own 128 x 64 output pixels of one pair, the
// staged rows start on 16-byte boundaries of the image row, 16-byte global accesses wherever W % 16 == 0 and the pointers
// are aligned (byte accesses otherwise), floor(log2 k) + 1 steps per direction on four pixels per lane, ping-pong between
// two LDS buffers.  The byte form was built rather than bit-packed rows: it reuses a scheme whose every index bound the
// suite already pins at k = 3 .. 63, and at 3 stencil passes per pair it costs what 1.5 launches of tpiv_prefilter cost.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));
typedef uint8_t u8x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTW = PREFILTER_TILE_COLS, kTH = PREFILTER_TILE_ROWS;
constexpr int kRMax = 31;
constexpr int kPitchMax = kTW + 2 * 32;                    // staged row: tile + two halos of r rounded up to 16
constexpr int kRowsMax = kTH + 2 * kRMax;
// one LDS buffer: the staged bytes [kRowsMax][kPitchMax] plus the slack that the doubling steps read past a buffer's last
// used dword (never into a result)
constexpr int kBufBytes = kRowsMax * kPitchMax + 64;
static_assert((kRowsMax + 16) * kTW <= kBufBytes, "the column steps read up to 16 rows past the staged ones");
static_assert(2 * kThreads == kTH * (kTW / 16), "a lane owns two chunks of 16 output pixels");

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ inline uint32_t min4(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u8x4, a), __builtin_bit_cast(u8x4, b)));
}

// the four bytes at byte offset off (any alignment) of an LDS buffer
__device__ inline uint32_t load4(const uint32_t* buf, int off) {
    const int d = off >> 2;
    return __builtin_amdgcn_alignbyte(buf[d + 1], buf[d], (uint32_t)(off & 3));
}

enum { kBright = 0, kDark = 1, kInvert = 2 };

// 0xFF where the pixel passes, 0x00 elsewhere: g >= level (kBright), g <= level (kDark), g == 0 (kInvert: ~core)
__device__ inline u8x16 binarise(u8x16 v, int how, uint8_t level) {
    const u8x16 lv = level;
    if (how == kBright) return __builtin_convertvector(v >= lv, u8x16);
    if (how == kDark) return __builtin_convertvector(v <= lv, u8x16);
    return __builtin_convertvector(v == (u8x16)(0), u8x16);
}

// Stage rows [y0 - r, y0 + th + r) x columns [x0 - hx, x0 + kTW + hx) of image f, binarised, into s; pixels outside the
// image as 0xFF.
template <bool kVec>
__device__ inline void stage(const uint8_t* __restrict__ f, int H, int W, int y0, int x0, int r, int hx, int rows, int pitch,
                             int how, uint8_t level, uint8_t* s) {
    const int chunks_row = pitch >> 4;
    const int chunks = rows * chunks_row;
    for (int c = threadIdx.x; c < chunks; c += kThreads) {
        const int sy = c / chunks_row, cx = c - sy * chunks_row;
        const int gy = y0 - r + sy, gx = x0 - hx + 16 * cx;
        u8x16 v = (uint8_t)255;
        if (gy >= 0 && gy < H) {
            const long long o = (long long)gy * W + gx;
            if constexpr (kVec) {                                   // W % 16 == 0: a chunk is inside or outside as a whole
                if (gx >= 0 && gx < W) v = binarise(*reinterpret_cast<const u8x16*>(f + o), how, level);
            } else {
                u8x16 px = (uint8_t)0;
                u8x16 in = (uint8_t)0;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (gx + j >= 0 && gx + j < W) {
                        px[j] = f[o + j];
                        in[j] = 255;
                    }
                }
                v = (binarise(px, how, level) & in) | ~in;
            }
        }
        *reinterpret_cast<u8x16*>(s + sy * pitch + 16 * cx) = v;
    }
}

// 16 bytes of row gy of an image from column gx on (0 past the row's end)
template <bool kVec>
__device__ inline u8x16 load16(const uint8_t* __restrict__ img, int W, int gy, int gx) {
    u8x16 v = (uint8_t)0;
    if (gx >= W) return v;
    const uint8_t* src = img + (long long)gy * W + gx;
    if constexpr (kVec) {
        v = *reinterpret_cast<const u8x16*>(src);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (gx + j < W) v[j] = src[j];
    }
    return v;
}

template <bool kVec>
__device__ inline void store16(uint8_t* __restrict__ out, int W, int gy, int gx, u8x16 v) {
    if (gx >= W) return;
    uint8_t* dst = out + (long long)gy * W + gx;
    if constexpr (kVec) {
        *reinterpret_cast<u8x16*>(dst) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (gx + j < W) dst[j] = v[j];
    }
}

// The sliding minimum over the k x k window of what lds[0] holds staged (prefilter_min_kernel's steps): this lane's two
// chunks of 16 output pixels into m[0], m[1].  Ends behind a barrier: lds[0] may be staged again.
__device__ inline void window_min(uint8_t (*lds)[kBufBytes], int k, int r, int hx, int pitch, int rows, int th, u8x16* m) {
    int p = 2;
    while (2 * p <= k) p *= 2;                                      // the largest power of two <= k
    int cur = 0;
    // rows: m_2s[i] = min(m_s[i], m_s[i + s]) over the staged bytes as one array (what runs into the next row lands
    // where no window reads)
    const int dwords = rows * pitch >> 2;
    for (int s = 1; s < p; s *= 2) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(lds[cur]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds[cur ^ 1]);
        for (int i = threadIdx.x; i < dwords; i += kThreads) dst[i] = min4(src[i], load4(src, 4 * i + s));
        cur ^= 1;
        __syncthreads();
    }
    {   // the window [x - r, x + r] = two spans of p, into rows of kTW
        const uint32_t* src = reinterpret_cast<const uint32_t*>(lds[cur]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds[cur ^ 1]);
        const int outs = rows * (kTW >> 2);
        for (int i = threadIdx.x; i < outs; i += kThreads) {
            const int sy = i / (kTW >> 2), xd = i - sy * (kTW >> 2);
            const int o = sy * pitch + hx - r + 4 * xd;
            dst[i] = min4(load4(src, o), load4(src, o + k - p));
        }
        cur ^= 1;
        __syncthreads();
    }
    // columns: the same on rows of kTW bytes, where every shift is a whole number of dwords
    const int cdwords = rows * (kTW >> 2);
    for (int s = 1; s < p; s *= 2) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(lds[cur]);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lds[cur ^ 1]);
        for (int i = threadIdx.x; i < cdwords; i += kThreads) dst[i] = min4(src[i], src[i + s * (kTW >> 2)]);
        cur ^= 1;
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = threadIdx.x + j * kThreads, yo = c >> 3, cx = c & 7;
        m[j] = (uint8_t)0;
        if (yo < th) {
            const u8x16 lo = *reinterpret_cast<const u8x16*>(lds[cur] + yo * kTW + 16 * cx);
            const u8x16 hi = *reinterpret_cast<const u8x16*>(lds[cur] + (yo + k - p) * kTW + 16 * cx);
            m[j] = __builtin_elementwise_min(lo, hi);
        }
    }
    __syncthreads();
}

// core[f] = erode(a[f]) | erode(b[f]), bytes 0x00 / 0xFF
template <bool kVec>
__global__ __launch_bounds__(kThreads) void dynmask_erode_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                  int n, int H, int W, int how, int k, int level,
                                                                  uint8_t* __restrict__ core) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kBufBytes];
    const int r = k >> 1, hx = (r + 15) & ~15, pitch = kTW + 2 * hx;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int th = H - y0 < kTH ? H - y0 : kTH, rows = th + 2 * r;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const long long fo = (long long)f * H * W;
        u8x16 acc[2], m[2];
        acc[0] = acc[1] = (uint8_t)0;
        for (int side = 0; side < 2; ++side) {
            stage<kVec>((side ? b : a) + fo, H, W, y0, x0, r, hx, rows, pitch, how, (uint8_t)level, lds[0]);
            __syncthreads();
            window_min(lds, k, r, hx, pitch, rows, th, m);
            acc[0] |= m[0];
            acc[1] |= m[1];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = threadIdx.x + j * kThreads, yo = c >> 3, cx = c & 7;
            if (yo < th) store16<kVec>(core + fo, W, y0 + yo, x0 + 16 * cx, acc[j]);
        }
    }
}

// out[f] = dilate(core[f]) | (fixed != 0), bytes 0 / 1; k = 2 (r + grow) + 1
template <bool kVec>
__global__ __launch_bounds__(kThreads) void dynmask_dilate_kernel(const uint8_t* __restrict__ core, int n, int H, int W, int k,
                                                                   const uint8_t* __restrict__ fixed,
                                                                   uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kBufBytes];
    const int r = k >> 1, hx = (r + 15) & ~15, pitch = kTW + 2 * hx;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int th = H - y0 < kTH ? H - y0 : kTH, rows = th + 2 * r;
    const u8x16 one = (uint8_t)1, zero = (uint8_t)0;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const long long fo = (long long)f * H * W;
        u8x16 m[2];
        stage<kVec>(core + fo, H, W, y0, x0, r, hx, rows, pitch, kInvert, 0, lds[0]);
        __syncthreads();
        window_min(lds, k, r, hx, pitch, rows, th, m);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = threadIdx.x + j * kThreads, yo = c >> 3, cx = c & 7;
            if (yo < th) {
                u8x16 v = __builtin_convertvector(m[j] == zero, u8x16);
                if (fixed) v |= __builtin_convertvector(load16<kVec>(fixed, W, y0 + yo, x0 + 16 * cx) != zero, u8x16);
                store16<kVec>(out + fo, W, y0 + yo, x0 + 16 * cx, v & one);
            }
        }
    }
}

}  // namespace

hipError_t launch_dynamic_mask(const uint8_t* a, const uint8_t* b, int n, int H, int W, int kind, int size, int level,
                               int grow, const uint8_t* fixed, uint8_t* out, uint8_t* core, hipStream_t stream) {
    if (n <= 0 || H <= 0 || W <= 0) return hipSuccess;
    if (kind != DYNMASK_BRIGHT && kind != DYNMASK_DARK) return hipErrorInvalidValue;
    if (size < 3 || size > 2 * kRMax + 1 || size % 2 == 0) return hipErrorInvalidValue;
    if (level < 0 || level > 255 || grow < 0 || size / 2 + grow > kRMax) return hipErrorInvalidValue;
    const int tx = (W + kTW - 1) / kTW, ty = (H + kTH - 1) / kTH;
    if (ty > 65535) return hipErrorInvalidValue;
    const dim3 grid(tx, ty, n < 65535 ? n : 65535);
    const bool vec = W % 16 == 0 && aligned16(a) && aligned16(b) && aligned16(core) && aligned16(out) &&
                     (!fixed || aligned16(fixed));
    const int how = kind == DYNMASK_BRIGHT ? kBright : kDark;
    if (vec)
        hipLaunchKernelGGL(dynmask_erode_kernel<true>, grid, dim3(kThreads), 0, stream, a, b, n, H, W, how, size, level, core);
    else
        hipLaunchKernelGGL(dynmask_erode_kernel<false>, grid, dim3(kThreads), 0, stream, a, b, n, H, W, how, size, level, core);
    if (hipError_t e = hipGetLastError()) return e;
    const int kd = 2 * (size / 2 + grow) + 1;
    if (vec)
        hipLaunchKernelGGL(dynmask_dilate_kernel<true>, grid, dim3(kThreads), 0, stream, core, n, H, W, kd, fixed, out);
    else
        hipLaunchKernelGGL(dynmask_dilate_kernel<false>, grid, dim3(kThreads), 0, stream, core, n, H, W, kd, fixed, out);
    return hipGetLastError();
}

}  // namespace tpiv
