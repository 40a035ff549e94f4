// Order-preserving compaction on the device, "count, scan, write in order": the pieces that the mesh, mask, raster and quantile kernels share.
//   count    every workgroup counts its kept items: wave_total or a ballot's popcount, then waves_before for the workgroup's sum -> sums[workgroup]
//   scan     scan_sums_kernel turns the sums into exclusive offsets in place and writes their total
//   write    the count pass again; an item's position = its workgroup's offset + block_excl / block_excl_flag of the items before it
// Integer work throughout and no atomic decides a position: the same bytes every run.  Workgroups are one-dimensional and a multiple of ADA_WAVE wide.
// Everything here has internal linkage: each translation unit that launches scan_sums_kernel keeps its own copy (the library is built -fno-gpu-rdc).
#pragma once
#include "ada_common.h"

namespace {

constexpr int ADA_WAVE = 64;

// Set bits of the ballot that belong to the lanes below this one.  No barrier; any lane may call it alone.
ADA_DEV int lanes_below(uint64_t ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// Inclusive prefix sum of v over the wave's lanes in order; lane ADA_WAVE - 1 holds the wave's total.  No barrier; every lane of the wave calls it.
template <typename T>
ADA_DEV T wave_incl_scan(T v) {
    const int lane = threadIdx.x & (ADA_WAVE - 1);
    T incl = v;
#pragma unroll
    for (int d = 1; d < ADA_WAVE; d <<= 1) {
        const T o = __shfl_up(incl, d, ADA_WAVE);
        if (lane >= d) incl += o;
    }
    return incl;
}

// Sum of v over the wave, in every lane.  No barrier; every lane of the wave calls it.
ADA_DEV int wave_total(int v) {
#pragma unroll
    for (int d = ADA_WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, ADA_WAVE);
    return v;
}

// The workgroup's WAVES waves exchange their totals through lds[WAVES]: returns the sum of the waves before this one, and the workgroup's sum in
// `total`.  `wave_sum` is read from the wave's LAST lane only (where wave_incl_scan leaves it; a popcount or wave_total is the same in every lane).
// TWO barriers, and EVERY thread of the workgroup calls it, under uniform control flow: the leading barrier waits for the readers of the previous
// call, so it may be called in a loop on the same array; the second one publishes the totals.  It orders nothing but `lds`.
template <int WAVES>
ADA_DEV int waves_before(int* lds, int wave_sum, int& total) {
    const int wave = threadIdx.x / ADA_WAVE;
    __syncthreads();
    if ((threadIdx.x & (ADA_WAVE - 1)) == ADA_WAVE - 1) lds[wave] = wave_sum;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const int t = lds[k];
        before += k < wave ? t : 0;
        total += t;
    }
    return before;
}

// Exclusive prefix of v over the workgroup's threads in order, and the workgroup's sum.  Barriers and calling rule: waves_before's.
template <int WAVES>
ADA_DEV int block_excl(int v, int* lds, int& total) {
    const int incl = wave_incl_scan(v);
    return waves_before<WAVES>(lds, incl, total) + incl - v;
}

// The same for a flag per thread, one ballot per wave: the set flags of the threads before this one.  Barriers and calling rule: waves_before's.
template <int WAVES>
ADA_DEV int block_excl_flag(bool f, int* lds, int& total) {
    const uint64_t bal = __ballot(f);
    return waves_before<WAVES>(lds, __popcll(bal), total) + lanes_below(bal);
}

// sums[row][0 .. n) -> exclusive prefix sums in place, total[row] = their sum; row = blockIdx.x, its sums start at sums + row * stride.  One workgroup
// of SCAN_THREADS per row; a step takes SCAN_THREADS * ITEMS sums, ITEMS consecutive ones per thread, and the running sum is carried from step to step.
constexpr int SCAN_THREADS = 1024;
template <int ITEMS>
__global__ __launch_bounds__(SCAN_THREADS) void scan_sums_kernel(int32_t* sums, long n, long stride, int32_t* total) {
    __shared__ int lds[SCAN_THREADS / ADA_WAVE];
    int32_t* s = sums + (long)blockIdx.x * stride;
    int carry = 0;
    for (long base = 0; base < n; base += (long)SCAN_THREADS * ITEMS) {
        const long i0 = base + (long)threadIdx.x * ITEMS;
        int v[ITEMS];
        int mine = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            v[k] = i0 + k < n ? s[i0 + k] : 0;
            mine += v[k];
        }
        int all;
        int run = carry + block_excl<SCAN_THREADS / ADA_WAVE>(mine, lds, all);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (i0 + k < n) s[i0 + k] = run;
            run += v[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

}  // namespace
