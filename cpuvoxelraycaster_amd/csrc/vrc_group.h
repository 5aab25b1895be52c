// vrc_group.h -- wave and workgroup primitives for 64-lane waves: the reductions and the exclusive scan of one value per
// lane over a wave, the sum and the exclusive scan of one 32-bit value per lane over a workgroup of WAVES waves, and the
// single-workgroup scan over an array of slots that turns per-workgroup counts into offsets.  Wave shuffles first, then one
// LDS word per wave; every function ends with its LDS free again.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t SCAN_GROUP = 1024;         // lanes of the workgroup that runs scan_slots: slots per step

// v summed / its least / its greatest over the 64 lanes of the wave, on every lane; called by whole waves
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int o = 32; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int o = 32; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// the sum of v over the lanes of the wave up to and including this one
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}
// the sum of v over the lanes of the wave before this one
__device__ __forceinline__ uint32_t wave_exclusive_scan(uint32_t v) { return wave_inclusive_scan(v) - v; }

// v summed over the lanes of a workgroup of WAVES waves, on every lane.  part: WAVES words of LDS, free again on return.
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t group_sum(uint32_t v, uint32_t* part)
{
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0u;
    for (uint32_t k = 0; k < WAVES; ++k) s += part[k];
    __syncthreads();
    return s;
}

// the sum of v over the lanes before this one, in a workgroup of WAVES waves; *total = the sum over all of them
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t group_exclusive_scan(uint32_t v, uint32_t* part, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(v);
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t k = 0; k < WAVES; ++k) {
        const uint32_t p = part[k];
        if (k < wave) before += p;
        all += p;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// slots[0 .. n_slots) -> their exclusive prefix, in place, by ONE workgroup of SCAN_GROUP lanes; returns the total (the
// carry behind the last slot).  A slot and the sum of the SCAN_GROUP slots of a step fit 32 bits; the prefix is a T.
template <class T>
__device__ __forceinline__ T scan_slots(T* __restrict__ slots, uint32_t n_slots)
{
    __shared__ uint32_t part[SCAN_GROUP / 64u];
    T carry = 0;
    for (uint32_t base = 0; base < n_slots; base += SCAN_GROUP) {      // uniform trip count
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_slots ? (uint32_t)slots[i] : 0u;
        uint32_t step = 0u;
        const uint32_t before = group_exclusive_scan<SCAN_GROUP / 64u>(v, part, &step);
        if (i < n_slots) slots[i] = carry + before;
        carry += step;
    }
    return carry;
}

// slots[0 .. n_slots) -> their exclusive prefix, slots[n_slots] = the total, also into *total_out unless that is null.
// Launched as ONE workgroup of SCAN_GROUP lanes.  The bound on a slot that scan_slots asks for is the caller's to state.
template <class T>
__global__ __launch_bounds__(SCAN_GROUP) void k_scan_slots(T* __restrict__ slots, uint32_t n_slots, T* __restrict__ total_out)
{
    const T total = scan_slots(slots, n_slots);
    if (threadIdx.x == 0) {
        slots[n_slots] = total;
        if (total_out) *total_out = total;
    }
}

}  // namespace
