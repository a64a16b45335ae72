// Deep (10..16-bit) frames on the device: the exact histogram of a recording's samples, and the tone map that turns
// uint16 samples into the uint8 frames every other kernel of the library reads.  The map is a table built on the host
// (engine.depth_lut: any curve, no new kernel) and the device only gathers, so the result is defined bit for bit by
// out = lut[src].
//
// LDS budget (160 KiB per CU).  The map keeps the whole 64 KiB table in LDS -- it does not fit the vector L1, and a
// gather from global memory per pixel would make a streaming kernel latency-bound -- so two workgroups of 1024 lanes
// share a CU (128 KiB, 8 wavefronts per SIMD); they are persistent and walk the frames grid-stride, so the 64 KiB
// table load is paid once per workgroup and not once per tile.  The histogram privatises all 65536 bins in LDS as
// packed 16-bit counters, two per dword: 128 KiB, one workgroup per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

constexpr int kThreads = 1024;
constexpr int kBins = 65536;
// samples a workgroup counts between two flushes of its private counters: no more than a 16-bit counter holds, and a
// multiple of 8 so that a 16-byte aligned source stays 16-byte aligned chunk after chunk
constexpr int kHistChunk = 65528;
static_assert(kHistChunk <= 65535 && kHistChunk % 8 == 0, "a private counter is 16 bits wide");

__device__ __forceinline__ uint32_t gather4(const uint8_t* tab, uint32_t lo, uint32_t hi) {
    return (uint32_t)tab[lo & 0xffffu] | ((uint32_t)tab[lo >> 16] << 8) | ((uint32_t)tab[hi & 0xffffu] << 16) |
           ((uint32_t)tab[hi >> 16] << 24);
}

__device__ __forceinline__ uint2 gather8(const uint8_t* tab, uint4 v) {
    return make_uint2(gather4(tab, v.x, v.y), gather4(tab, v.z, v.w));
}

// out[f][p] = lut[src[off[f] + p]] (off == nullptr: f * pixels).  A frame whose source is 16-byte aligned and whose
// output is 8-byte aligned moves as 16-byte loads of 8 samples and 8-byte stores, two of them in flight per lane, its
// pixels % 8 tail sample by sample; any other frame (odd widths, odd slot offsets, tensor views) sample by sample as a
// whole.  The choice is per frame and uniform over the grid.
__global__ __launch_bounds__(kThreads) void depth_map_kernel(const uint16_t* __restrict__ src, const long long* __restrict__ off,
                                                             int n, long long pixels, const uint8_t* __restrict__ lut,
                                                             uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[kBins];
    if (((uintptr_t)lut & 15u) == 0) {
        for (int i = threadIdx.x; i < kBins / 16; i += kThreads)
            reinterpret_cast<uint4*>(tab)[i] = reinterpret_cast<const uint4*>(lut)[i];
    } else {
        for (int i = threadIdx.x; i < kBins; i += kThreads) tab[i] = lut[i];
    }
    __syncthreads();
    const long long stride = (long long)gridDim.x * kThreads;
    const long long t0 = (long long)blockIdx.x * kThreads + threadIdx.x;
    for (int f = 0; f < n; ++f) {
        const uint16_t* __restrict__ sp = src + (off ? off[f] : (long long)f * pixels);
        uint8_t* __restrict__ op = out + (long long)f * pixels;
        if ((((uintptr_t)sp & 15u) | ((uintptr_t)op & 7u)) == 0) {
            const uint4* __restrict__ s8 = reinterpret_cast<const uint4*>(sp);
            uint2* __restrict__ o8 = reinterpret_cast<uint2*>(op);
            const long long full = pixels / 8;
            long long g = t0;
            for (; g + stride < full; g += 2 * stride) {
                const uint4 v0 = s8[g], v1 = s8[g + stride];
                o8[g] = gather8(tab, v0);
                o8[g + stride] = gather8(tab, v1);
            }
            if (g < full) o8[g] = gather8(tab, s8[g]);
            const long long p = full * 8 + t0;
            if (p < pixels) op[p] = tab[sp[p]];
        } else {
            for (long long p = t0; p < pixels; p += stride) op[p] = tab[sp[p]];
        }
    }
}

__device__ __forceinline__ void count(uint32_t* cnt, uint32_t v) { atomicAdd(&cnt[v >> 1], 1u << ((v & 1u) * 16)); }

// hist[v] += the number of samples of src[0 .. total) that equal v.  A workgroup takes chunks of kHistChunk samples:
// it counts a chunk into its private 16-bit counters (LDS atomics; bins 2k and 2k + 1 share dword k, and with at most
// 65535 samples per chunk neither half can carry into the other), then adds the counters that are not zero to the
// 64-bit global bins and clears them.  A dark frame touches a few hundred bins, so a flush is a few hundred global
// atomics per 65528 samples whatever the contention inside the chunk was.
__global__ __launch_bounds__(kThreads) void depth_histogram_kernel(const uint16_t* __restrict__ src, long long total,
                                                                   unsigned long long* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[kBins / 2];
    for (int i = threadIdx.x; i < kBins / 8; i += kThreads) reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const long long chunks = (total + kHistChunk - 1) / kHistChunk;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint16_t* __restrict__ p = src + c * kHistChunk;
        const long long left = total - c * kHistChunk;
        const int len = left < kHistChunk ? (int)left : kHistChunk;
        // samples in front of the first 16-byte boundary (src is 2-byte aligned), 16-byte groups, samples behind them
        int head = (int)(((16u - ((uintptr_t)p & 15u)) & 15u) / 2);
        head = head < len ? head : len;
        const int groups = (len - head) / 8;
        const int tail = head + groups * 8;
        if ((int)threadIdx.x < head) count(cnt, p[threadIdx.x]);
        const uint4* __restrict__ p8 = reinterpret_cast<const uint4*>(p + head);
        for (int g = threadIdx.x; g < groups; g += kThreads) {
            const uint4 v = p8[g];
            count(cnt, v.x & 0xffffu);
            count(cnt, v.x >> 16);
            count(cnt, v.y & 0xffffu);
            count(cnt, v.y >> 16);
            count(cnt, v.z & 0xffffu);
            count(cnt, v.z >> 16);
            count(cnt, v.w & 0xffffu);
            count(cnt, v.w >> 16);
        }
        if (tail + (int)threadIdx.x < len) count(cnt, p[tail + threadIdx.x]);       // (fewer than 8 of them)
        __syncthreads();
        for (int i = threadIdx.x; i < kBins / 8; i += kThreads) {
            const uint4 w = reinterpret_cast<uint4*>(cnt)[i];
            if ((w.x | w.y | w.z | w.w) == 0) continue;
            reinterpret_cast<uint4*>(cnt)[i] = make_uint4(0, 0, 0, 0);
            const uint32_t word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (word[k] & 0xffffu) atomicAdd(&hist[8 * i + 2 * k], (unsigned long long)(word[k] & 0xffffu));
                if (word[k] >> 16) atomicAdd(&hist[8 * i + 2 * k + 1], (unsigned long long)(word[k] >> 16));
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_depth_map(const uint16_t* src, const long long* src_off, int n, int H, int W, const uint8_t* lut,
                            uint8_t* out, int n_cu, hipStream_t stream) {
    if (n <= 0 || H <= 0 || W <= 0) return hipSuccess;
    const long long pixels = (long long)H * W;
    const long long want = (pixels + kThreads - 1) / kThreads;          // a lane per sample at most
    const long long most = 2LL * (n_cu > 0 ? n_cu : 1);                 // two workgroups per CU (64 KiB of LDS each)
    const unsigned blocks = (unsigned)(want < most ? want : most);
    hipLaunchKernelGGL(depth_map_kernel, dim3(blocks), dim3(kThreads), 0, stream, src, src_off, n, pixels, lut, out);
    return hipGetLastError();
}

hipError_t launch_depth_histogram(const uint16_t* src, long long total, unsigned long long* hist, int n_cu,
                                  hipStream_t stream) {
    if (total <= 0) return hipSuccess;
    const long long chunks = (total + kHistChunk - 1) / kHistChunk;
    const long long most = n_cu > 0 ? n_cu : 1;                         // one workgroup per CU (128 KiB of LDS)
    const unsigned blocks = (unsigned)(chunks < most ? chunks : most);
    hipLaunchKernelGGL(depth_histogram_kernel, dim3(blocks), dim3(kThreads), 0, stream, src, total, hist);
    return hipGetLastError();
}

}  // namespace tpiv
