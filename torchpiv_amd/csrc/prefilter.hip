// Spatial pre-filters on the device: sliding-minimum subtraction, local-mean high-pass and intensity capping of uint8
// frames, with the static background (background.hip) subtracted on the way in.  Integer in, integer out, every step as
// tests/prefilter_model.py states it, so the result is that model's bit for bit and every correlation kernel and
// precision applies to the filtered frames unchanged.
//
// Per frame f [H, W], odd size k = 2r + 1 in 3..63, g = max(f, bg) - bg (g = f without a background):
//   min:   out = g - min(k x k neighbourhood of g, clipped to the image)
//   mean:  S = sum over that neighbourhood, c = its pixel count, m = (2S + c) / (2c), out = max(g - m, 0)
//   cap:   out = min(out, cap), last; alone (kind none): out = min(g, cap), a streaming kernel.
//
// The stencil kernels: a workgroup of 256 lanes owns a tile of kTW x kTH = 128 x 64 output pixels of one frame and
// stages it with its halo in LDS as bytes: r rows above and below, hx = r rounded up to 16 columns left and right, so
// that every staged row starts on a 16-byte boundary of the image row and global loads are 16 bytes per lane wherever
// W % 16 == 0 and the pointers are aligned (otherwise the same lanes load byte by byte).  Pixels outside the image are
// staged as the neutral value (255 for the minimum, 0 for the sum; c is computed from the coordinates), so no later
// step knows about the border.  Rows first, then columns, both out of LDS:
//   min:  doubling, four pixels (one dword) per lane and step: m1[i] = min(x[i], x[i+1]), m2[i] = min(m1[i], m1[i+2]),
//         ... up to the largest power of two p <= k, then min(mp[i], mp[i + k - p]) -- floor(log2 k) + 1 steps per
//         direction, ping-pong between two LDS buffers.  A step that shifts by a byte count that is no multiple of 4
//         funnels two dwords (v_alignbyte).
//   mean: running sums: a lane per staged column walks down the rows (16-bit column sums), then a lane per 32 output
//         pixels of a row walks along those (32-bit).  2 additions per pixel and direction plus the k of a walk's start.
// The work that does grow with k is the halo's: (kTH + 2r)(kTW + 2hx) staged pixels per kTH x kTW tile, 1.3x at k = 3 and
// 2.95x at k = 63.
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
// one LDS buffer: the staged bytes [kRowsMax][kPitchMax] or the 16-bit column sums [kTH][kPitchMax], whichever is larger,
// plus the slack that the doubling steps read past a buffer's last used dword (never into a result)
constexpr int kBufBytes = (kRowsMax * kPitchMax > 2 * kTH * kPitchMax ? kRowsMax * kPitchMax : 2 * kTH * kPitchMax) + 64;
static_assert(kThreads == 4 * kTH && kTW == 4 * 32, "mean: a lane per 32 output pixels of a row");
static_assert(kThreads >= kPitchMax, "mean: a lane per staged column");
static_assert((kRowsMax + 16) * kTW <= kBufBytes, "min: the column steps read up to 16 rows past the staged ones");

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ inline uint32_t min4(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u8x4, a), __builtin_bit_cast(u8x4, b)));
}

// the four bytes at byte offset off (any alignment) of an LDS buffer
__device__ inline uint32_t load4(const uint32_t* buf, int off) {
    const int d = off >> 2;
    return __builtin_amdgcn_alignbyte(buf[d + 1], buf[d], (uint32_t)(off & 3));
}

// Stage rows [y0 - r, y0 + th + r) x columns [x0 - hx, x0 + kTW + hx) of frame f (minus the background) into s, pixels
// outside the image as `neutral`.
template <bool kVec>
__device__ inline void stage(const uint8_t* __restrict__ f, const uint8_t* __restrict__ bg, int H, int W, int y0, int x0,
                             int r, int hx, int rows, int pitch, uint8_t neutral, uint8_t* s) {
    const int chunks_row = pitch >> 4;
    const int chunks = rows * chunks_row;
    for (int c = threadIdx.x; c < chunks; c += kThreads) {
        const int sy = c / chunks_row, cx = c - sy * chunks_row;
        const int gy = y0 - r + sy, gx = x0 - hx + 16 * cx;
        u8x16 v = neutral;
        if (gy >= 0 && gy < H) {
            const long long o = (long long)gy * W + gx;
            if constexpr (kVec) {                                   // W % 16 == 0: a chunk is inside or outside as a whole
                if (gx >= 0 && gx < W) {
                    v = *reinterpret_cast<const u8x16*>(f + o);
                    if (bg) v = __builtin_elementwise_sub_sat(v, *reinterpret_cast<const u8x16*>(bg + o));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (gx + j >= 0 && gx + j < W) {
                        const uint8_t p = f[o + j], b = bg ? bg[o + j] : (uint8_t)0;
                        v[j] = p > b ? (uint8_t)(p - b) : (uint8_t)0;
                    }
                }
            }
        }
        *reinterpret_cast<u8x16*>(s + sy * pitch + 16 * cx) = v;
    }
}

// 16 output pixels of row gy from column gx on
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

template <bool kVec>
__global__ __launch_bounds__(kThreads) void prefilter_min_kernel(const uint8_t* __restrict__ frames, int n, int H, int W,
                                                                  const uint8_t* __restrict__ bg, int k, int cap,
                                                                  uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kBufBytes];
    const int r = k >> 1, hx = (r + 15) & ~15, pitch = kTW + 2 * hx;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int th = H - y0 < kTH ? H - y0 : kTH, rows = th + 2 * r;
    int p = 2;
    while (2 * p <= k) p *= 2;                                      // the largest power of two <= k
    const u8x16 capv = (uint8_t)cap;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const long long fo = (long long)f * H * W;
        stage<kVec>(frames + fo, bg, H, W, y0, x0, r, hx, rows, pitch, 255, lds[0]);
        __syncthreads();
        // this lane's output pixels (two chunks of 16), kept while the buffers are overwritten
        u8x16 g[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = threadIdx.x + j * kThreads, yo = c >> 3, cx = c & 7;
            g[j] = yo < th ? *reinterpret_cast<const u8x16*>(lds[0] + (yo + r) * pitch + hx + 16 * cx) : u8x16(0);
        }
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
            if (yo < th) {
                const u8x16 lo = *reinterpret_cast<const u8x16*>(lds[cur] + yo * kTW + 16 * cx);
                const u8x16 hi = *reinterpret_cast<const u8x16*>(lds[cur] + (yo + k - p) * kTW + 16 * cx);
                u8x16 v = g[j] - __builtin_elementwise_min(lo, hi);
                v = __builtin_elementwise_min(v, capv);
                store16<kVec>(out + fo, W, y0 + yo, x0 + 16 * cx, v);
            }
        }
        __syncthreads();                                            // the next frame stages into what was just read
    }
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void prefilter_mean_kernel(const uint8_t* __restrict__ frames, int n, int H, int W,
                                                                   const uint8_t* __restrict__ bg, int k, int cap,
                                                                   uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][kBufBytes];
    const int r = k >> 1, hx = (r + 15) & ~15, pitch = kTW + 2 * hx;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int th = H - y0 < kTH ? H - y0 : kTH, rows = th + 2 * r;
    const uint8_t* s = lds[0];
    uint16_t* col = reinterpret_cast<uint16_t*>(lds[1]);           // column sums [th][pitch]
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const long long fo = (long long)f * H * W;
        stage<kVec>(frames + fo, bg, H, W, y0, x0, r, hx, rows, pitch, 0, lds[0]);
        __syncthreads();
        if ((int)threadIdx.x < pitch) {                             // a lane per staged column: k rows, then slide
            const int x = threadIdx.x;
            uint32_t sum = 0;
            for (int j = 0; j < k; ++j) sum += s[j * pitch + x];
            for (int yo = 0; yo < th; ++yo) {
                col[yo * pitch + x] = (uint16_t)sum;                // <= 63 * 255
                if (yo + 1 < th) sum += (uint32_t)s[(yo + k) * pitch + x] - (uint32_t)s[yo * pitch + x];
            }
        }
        __syncthreads();
        const int yo = threadIdx.x >> 2, xs = (threadIdx.x & 3) * 32;
        if (yo < th) {                                              // a lane per 32 output pixels of a row
            const int gy = y0 + yo;
            const int cy = (gy + r < H - 1 ? gy + r : H - 1) - (gy - r > 0 ? gy - r : 0) + 1;
            const uint16_t* cr = col + yo * pitch + hx - r + xs;    // cr[x'] .. cr[x' + k - 1]: the window of pixel xs + x'
            const uint8_t* gr = s + (yo + r) * pitch + hx + xs;
            uint32_t sum = 0;
            for (int j = 0; j < k; ++j) sum += cr[j];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u8x16 v;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int xo = 16 * h + j, gx = x0 + xs + xo;
                    int cx = (gx + r < W - 1 ? gx + r : W - 1) - (gx - r > 0 ? gx - r : 0) + 1;
                    cx = cx > 0 ? cx : 1;                           // columns past the image: stored nowhere
                    const uint32_t c = (uint32_t)(cy * cx), num = 2 * sum + c, den = 2 * c;
                    // num / den exactly: num < 2^21 and the quotient <= 255, so the float estimate is off by at most one
                    uint32_t m = (uint32_t)((float)num * __builtin_amdgcn_rcpf((float)den));
                    if (m * den > num) --m;
                    if ((m + 1) * den <= num) ++m;
                    const uint32_t px = gr[xo];
                    uint32_t o = px > m ? px - m : 0;
                    o = o < (uint32_t)cap ? o : (uint32_t)cap;
                    v[j] = (uint8_t)o;
                    if (xo + 1 < 32) sum += (uint32_t)cr[xo + k] - (uint32_t)cr[xo];
                }
                store16<kVec>(out + fo, W, gy, x0 + xs + 16 * h, v);
            }
        }
        __syncthreads();
    }
}

// kind none: out = min(max(f, bg) - bg, cap), streaming like subtract_background_kernel (a lane owns 16 bytes of the image)
template <bool kVec>
__global__ __launch_bounds__(kThreads) void prefilter_cap_kernel(const uint8_t* __restrict__ frames, int n, long long pixels,
                                                                  const uint8_t* __restrict__ bg, int cap,
                                                                  uint8_t* __restrict__ out) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (p0 >= pixels) return;
    if constexpr (kVec) {
        const u8x16 b = bg ? *reinterpret_cast<const u8x16*>(bg + p0) : u8x16(0);
        const u8x16 capv = (uint8_t)cap;
        for (int f = blockIdx.y; f < n; f += gridDim.y) {
            const long long o = (long long)f * pixels + p0;
            const u8x16 v = __builtin_elementwise_sub_sat(*reinterpret_cast<const u8x16*>(frames + o), b);
            *reinterpret_cast<u8x16*>(out + o) = __builtin_elementwise_min(v, capv);
        }
    } else {
        const int cnt = pixels - p0 < 16 ? (int)(pixels - p0) : 16;
        for (int f = blockIdx.y; f < n; f += gridDim.y) {
            const long long o = (long long)f * pixels + p0;
            for (int j = 0; j < cnt; ++j) {
                const int b = bg ? bg[p0 + j] : 0, v = frames[o + j];
                const int d = v > b ? v - b : 0;
                out[o + j] = (uint8_t)(d < cap ? d : cap);
            }
        }
    }
}

}  // namespace

hipError_t launch_prefilter(const uint8_t* frames, int n, int H, int W, const uint8_t* bg, int kind, int size, int cap,
                            uint8_t* out, hipStream_t stream) {
    if (n <= 0 || H <= 0 || W <= 0) return hipSuccess;
    if (kind != PREFILTER_NONE && kind != PREFILTER_MIN && kind != PREFILTER_MEAN) return hipErrorInvalidValue;
    if (kind != PREFILTER_NONE && (size < 3 || size > 2 * kRMax + 1 || size % 2 == 0)) return hipErrorInvalidValue;
    if (cap < 1 || cap > 255) return hipErrorInvalidValue;
    const long long pixels = (long long)H * W;
    const bool al = aligned16(frames) && aligned16(out) && (!bg || aligned16(bg));
    if (kind == PREFILTER_NONE) {
        const long long blocks = ((pixels + 15) / 16 + kThreads - 1) / kThreads;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        const dim3 grid((unsigned)blocks, n < 65535 ? n : 65535);
        if (al && pixels % 16 == 0)
            hipLaunchKernelGGL(prefilter_cap_kernel<true>, grid, dim3(kThreads), 0, stream, frames, n, pixels, bg, cap, out);
        else
            hipLaunchKernelGGL(prefilter_cap_kernel<false>, grid, dim3(kThreads), 0, stream, frames, n, pixels, bg, cap, out);
        return hipGetLastError();
    }
    const int tx = (W + kTW - 1) / kTW, ty = (H + kTH - 1) / kTH;
    if (ty > 65535) return hipErrorInvalidValue;
    const dim3 grid(tx, ty, n < 65535 ? n : 65535);
    const bool vec = al && W % 16 == 0;
    auto kernel = kind == PREFILTER_MIN ? (vec ? prefilter_min_kernel<true> : prefilter_min_kernel<false>)
                                        : (vec ? prefilter_mean_kernel<true> : prefilter_mean_kernel<false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, frames, n, H, W, bg, size, cap, out);
    return hipGetLastError();
}

}  // namespace tpiv
