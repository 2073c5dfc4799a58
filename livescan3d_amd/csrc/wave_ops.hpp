// wave_ops.hpp -- the wave (64 lanes) and workgroup primitives every stage shares: scans, ranks and reductions.  Device code only.
// A stage that needs a prefix sum, a block rank or a wave reduction calls these; it does not write its own.
#pragma once

#include <hip/hip_runtime.h>

// Inclusive prefix sum over the wave's lanes (lane = threadIdx.x & 63).
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T n = __shfl_up(v, off, 64);
        if (lane >= off) v += n;
    }
    return v;
}

// The reductions are xor butterflies in the order off = 32 ... 1, valid in every lane.  For floating types that order is part of the
// result: wave_sum<double> feeds the ICP Kabsch sums, whose digests the tests pin.  Do not reorder it.
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// Inclusive prefix sum over a workgroup of WAVES whole waves, every thread calling; *total (when asked for) = the workgroup's sum, in
// every thread.  s_wave: WAVES entries of LDS.  One barrier before the waves' totals are read and one after: the caller may call again
// with the same s_wave, in a loop for instance, without a barrier of its own.
template <typename T, int WAVES>
__device__ __forceinline__ T block_scan_incl(T v, T *s_wave, T *total = nullptr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_scan_incl(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const T x = s_wave[w];
        pre += w < wave ? x : T(0);
        tot += x;
    }
    __syncthreads();
    if (total) *total = tot;
    return pre + incl;
}

// Exclusive rank of `flag` among the workgroup's threads (WAVES whole waves) from the lane masks, and the number of flags set.
// One barrier: s_wave (WAVES ints of LDS) is not to be rewritten before the caller's next one.
template <int WAVES>
__device__ __forceinline__ int block_rank(bool flag, int *s_wave, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0));
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        rank += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    return rank;
}

// One workgroup of THREADS threads: out[i] = in[0] + in[stride] + ... + in[(i - 1) * stride] for i < n, THREADS elements per round with the
// rounds' sum carried along; *grand_total (when asked for) = the sum of all n.  `out` may be `in` (stride 1); grand_total may be out + n.
template <typename T, int THREADS>
__device__ __forceinline__ void block_scan_array_excl(const T *in, long long stride, T *out, int n, T *s_wave /* THREADS / 64 */,
                                                      T *grand_total = nullptr)
{
    T carry = 0;   // uniform: every thread adds the same round totals
    for (int c0 = 0; c0 < n; c0 += THREADS) {
        const int i = c0 + (int)threadIdx.x;
        const T v = i < n ? in[i * stride] : T(0);
        T round;
        const T incl = block_scan_incl<T, THREADS / 64>(v, s_wave, &round);
        if (i < n) out[i] = carry + incl - v;
        carry += round;
    }
    if (grand_total && threadIdx.x == 0) *grand_total = carry;
}
