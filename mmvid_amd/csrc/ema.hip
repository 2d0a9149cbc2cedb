// Exponential moving average of the flat fp32 weights (engine.FlatTrainer: ema_decay).  include/mmvid_hip_ext.h states the rule;
// tests/ema_ref.py is its host replica, bit for bit.
//   t = step_dev ? *step_dev : (float)step          finished optimiser steps, this one included
//   d = warmup ? fminf(decay, (1 + t) / (10 + t)) : decay ;  a = 1 - d          one fp32 operation each
//   ema' = fmaf(a, p - ema, ema)                                                  exact where ema == p: the result is p
// HBM-bound like the Adam kernel it follows (csrc/optim.hip): 12 B per parameter (p and ema read, ema written), one launch for the
// whole model, 256 threads, float4, a grid-stride loop, a scalar tail for n % 4.  No atomics, no LDS.  A row of the lazy table
// (step_state.h: the table Adam got) whose flag is 0 is neither read nor written: the trainer keeps ema == p there, where the update
// is the identity.
// Two departures from the Adam kernel's loop, both measured at BERT's 124.7 M elements ("Weight EMA"): the grid is
// capped at 512 blocks, not 2,048 (0.300 ms at 2,048, 0.282 at 1,024, 0.268 at 512 with plain loads), and every byte is touched once
// per step, so loads and stores are nontemporal (0.229 ms at 512 blocks: 6.5 TB/s).  Unrolling the loop over two or four trips was
// slower (0.325 / 0.416 ms).
#include "../../include/mmvid_hip_ext.h"
#include "step_state.h"

namespace {

__device__ __forceinline__ float ema_one(float a, float p, float e) {
    const float diff = __fsub_rn(p, e);  // (an explicit fp32 subtraction: never contracted into the fmaf)
    return fmaf(a, diff, e);
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float decay, int warmup,
                                                  float t, const float* __restrict__ step_dev, LazyRows z,
                                                  const int* __restrict__ skip) {
    if (step_skipped(skip)) return;
    t = device_wins(step_dev, t);  // (a captured step follows the warm-up without host input)
    float d = decay;
    if (warmup) d = fminf(decay, __fdiv_rn(__fadd_rn(1.f, t), __fadd_rn(10.f, t)));
    const float a = __fsub_rn(1.f, d);
    const long stride = (long)gridDim.x * 256 * 4;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (lazy_skip(z, i)) continue;
        if (i + 3 < n) {
            const f32x4 pp = load_once(p + i), ee = load_once(ema + i);
            const f32x4 out = {ema_one(a, pp.x, ee.x), ema_one(a, pp.y, ee.y), ema_one(a, pp.z, ee.z), ema_one(a, pp.w, ee.w)};
            __builtin_nontemporal_store(out, reinterpret_cast<f32x4*>(ema + i));
        } else {
            for (long k = i; k < n; ++k) ema[k] = ema_one(a, p[k], ema[k]);
        }
    }
}

}  // namespace

// mmvid_ema_update (skip_dev NULL) and mmvid_ema_update_guarded: one set of checks, one kernel
static int ema_launch(float* ema, const float* p, int64_t n, float decay, int warmup, int step, const float* step_dev,
                      const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, const int32_t* skip_dev, void* stream) {
    MMVID_REQUIRE(ema && p, "ema_update: ema and p must not be NULL");
    MMVID_REQUIRE(n >= 0 && n <= (int64_t)1 << 60, "ema_update: n=%lld is negative (or beyond 2^60)", (long long)n);
    MMVID_REQUIRE((((uintptr_t)ema | (uintptr_t)p) & 15) == 0, "ema_update: buffers must be 16-byte aligned");
    {
        const uintptr_t e0 = (uintptr_t)ema, p0 = (uintptr_t)p, bytes = (uintptr_t)n * 4;
        MMVID_REQUIRE(e0 != p0 && (e0 < p0 ? p0 - e0 >= bytes : e0 - p0 >= bytes),
                      "ema_update: ema and p must not be the same buffer and must not overlap");
    }
    MMVID_REQUIRE(decay >= 0.f && decay < 1.f, "ema_update: decay=%g is outside [0, 1)", (double)decay);  // (false for NaN)
    MMVID_REQUIRE(step >= 1 || step_dev, "ema_update: step=%d must be >= 1 where no device step count is given", step);
    LazyRows z;
    if (int rc = make_lazy(z, "ema_update", row_flags, table_lo, table_rows, rowlen, n)) return rc;
    if (n == 0) return MMVID_OK;
    long b = (long)((n + 1023) / 1024);
    if (b > 512) b = 512;  // (two blocks per CU: see the head of this file)
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, ema, p, (long)n, decay, warmup != 0,
                       (float)(step >= 1 ? step : 1), step_dev, z, (const int*)skip_dev);
    MMVID_LAUNCH_CHECK("ema_update");
    return MMVID_OK;
}

extern "C" int mmvid_ema_update(float* ema, const float* p, int64_t n, float decay, int warmup, int step, const float* step_dev,
                                const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, void* stream) {
    return ema_launch(ema, p, n, decay, warmup, step, step_dev, row_flags, table_lo, table_rows, rowlen, nullptr, stream);
}

extern "C" int mmvid_ema_update_guarded(float* ema, const float* p, int64_t n, float decay, int warmup, int step, const float* step_dev,
                                        const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen,
                                        const int32_t* skip_dev, void* stream) {
    MMVID_REQUIRE(((uintptr_t)skip_dev & 3) == 0, "ema_update_guarded: skip_dev must be 4-byte aligned");
    return ema_launch(ema, p, n, decay, warmup, step, step_dev, row_flags, table_lo, table_rows, rowlen, skip_dev, stream);
}
