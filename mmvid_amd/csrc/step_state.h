// What the kernels of one optimiser step share (optim.hip: gradient norm, guard, Adam; telemetry.hip; ema.hip): the lazy table, the
// scalars a captured step reads from the device, and the loads of a buffer that is touched once per step.  Each rule is stated here
// once.  No expression of this header has a product that feeds a sum or a difference: telemetry.hip compiles with fp contraction off
// and optim.hip with it on, and both inline these functions.
#pragma once
#include <math.h>

#include "common.h"

// "Lazy rows": one table inside the flat buffers (elements [lo, lo + rows * rowlen)) whose rows carry a flag "has ever received
// a gradient".  A row that never did has g = m = v = 0, so Adam (without weight decay) leaves p, m, v unchanged and its g^2 is 0:
// skipping it is EXACT, and saves all 30 B per parameter.  The text embedding is 49,472 x 768 = 30 % of BERT's parameters and
// a step touches at most 3 * B * 64 of its rows (the engine sets the flags from the ids the model logged).  The telemetry and the
// EMA are exact on the same rows only because every kernel skips through lazy_skip, on a table make_lazy accepted.
struct LazyRows {
    const unsigned char* flags;  // null: no lazy table
    long lo, hi;                 // element range of the table in the flat buffer
    int rowlen;
};
// (rowlen % 4 == 0 and lo % 4 == 0: the four elements of an aligned float4 share a row)
__device__ __forceinline__ bool lazy_skip(const LazyRows& z, long i) {
    return z.flags && i >= z.lo && i < z.hi && z.flags[(i - z.lo) / z.rowlen] == 0;
}
// The host check of every entry that takes a table, made before the entry's n == 0 return.  n >= 0 is the caller's check.
static inline int make_lazy(LazyRows& z, const char* who, const uint8_t* flags, int64_t lo, int64_t rows, int rowlen, int64_t n) {
    z.flags = nullptr, z.lo = z.hi = 0, z.rowlen = 1;
    if (!flags) return MMVID_OK;
    MMVID_REQUIRE(lo >= 0 && rows >= 0 && rowlen > 0 && rowlen % 4 == 0 && lo % 4 == 0 && lo <= n && rows <= (n - lo) / rowlen,
                  "%s: lazy rows: the table [%lld, +%lld x %d) must lie inside the buffer and be 4-element aligned", who, (long long)lo,
                  (long long)rows, rowlen);
    z.flags = flags, z.lo = lo, z.hi = lo + rows * rowlen, z.rowlen = rowlen;
    return MMVID_OK;
}

// A step scalar kept on the device (the learning rate of mmvid_lr_schedule, the step count) wins over the launch's host value: a
// captured step follows the schedule and the count without host input.  A kernel argument's load, the same in every lane.
__device__ __forceinline__ float device_wins(const float* dev, float host) { return dev ? *dev : host; }
// the verdict of the non-finite guard (mmvid_step_guard), null where the step is unguarded: a scalar branch
__device__ __forceinline__ bool step_skipped(const int* skip) { return skip && *skip; }
// false for inf and NaN: the exponent is all ones
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// Adam's bias corrections after t steps: on the host t = step >= 1 ? step : 1, in a kernel t = *step_dev
struct BiasCorrections {
    float bc1, bc2_sqrt;
};
__host__ __device__ __forceinline__ BiasCorrections bias_corrections(float beta1, float beta2, float t) {
    return {1.0f - powf(beta1, t), sqrtf(1.0f - powf(beta2, t))};
}

// The warm-up of deepspeed's WarmupLR and WarmupDecayLR (third-party: restated from its published semantics) after k scheduler
// steps, k < warmup: log(k + 1) / log(warmup), the warm-up length clamped to >= 2 as deepspeed clamps it.  Kind 1 of
// mmvid_lr_schedule and kind 4 of mmvid_lr_schedule_ext both take it from here.
__device__ __forceinline__ long warmup_clamped(long warmup) { return warmup < 2 ? 2 : warmup; }
__device__ __forceinline__ float warmup_log_gamma(long k, long warmup_clamped_) {
    return logf((float)(k + 1)) / logf((float)warmup_clamped_);
}

// a float4 of a buffer that is read once per step
__device__ __forceinline__ f32x4 load_once(const float* q) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q)); }
