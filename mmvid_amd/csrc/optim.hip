// Optimiser step over flat fp32 buffers (Adam + clip_grad_norm_, train.py:322-325,
// utils_train.py:167-172).  HBM-bound: 28 B read+written per parameter, one launch for the whole model.
//   grad_sqnorm : out[0] += sum g^2   (two-level reduction, fp32 atomics per block)
//   adam_step   : torch.optim.Adam semantics (no amsgrad, weight_decay optional as L2 added to grad):
//                 g *= clip_coef, clip_coef = min(1, max_norm / (sqrt(sqnorm) + 1e-6))   (clip_grad_norm_)
//                 m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
//                 p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
//                 also refreshes the bf16 shadow copy the MFMA kernels read.
#include "../../include/mmvid_hip.h"
#include "../../include/mmvid_hip_ext.h"
#include "step_state.h"

namespace {

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, long n,
                                                          float* __restrict__ out) {
    float a = 0.f;
    const long stride = (long)gridDim.x * 256 * 4;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            a += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        } else {
            for (long k = i; k < n; ++k) a += g[k] * g[k];
        }
    }
    a = wave_sum(a);
    __shared__ float sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(out, (sh[0] + sh[1]) + (sh[2] + sh[3]));
}

struct AdamArgs {
    float lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, max_norm, grad_scale;
};

// DECOUPLED (mmvid_adam_step_decoupled, torch.optim.AdamW): the decay leaves the gradient and scales the weight instead,
//     gr = g * coef ;  p' = p * keep - (lr / bc1) * m' / (sqrtf(v') / bc2s + eps) ,  keep = 1.f - lr * wd  (one scalar per launch)
// Everything else -- the scalars, the lazy rows, the verdict, the shadow -- is the one text below for both forms.
template <bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   bf16_t* __restrict__ shadow, long n, AdamArgs a,
                                                   const float* __restrict__ sqnorm,
                                                   const float* __restrict__ step_dev,
                                                   const float* __restrict__ lr_dev, LazyRows z,
                                                   const int* __restrict__ skip) {
    if (step_skipped(skip)) return;
    a.lr = device_wins(lr_dev, a.lr);
    if (step_dev) {  // (whole-step graph replay)
        const BiasCorrections bc = bias_corrections(a.beta1, a.beta2, *step_dev);
        a.bc1 = bc.bc1, a.bc2_sqrt = bc.bc2_sqrt;
    }
    float coef = a.grad_scale;
    if (sqnorm && a.max_norm > 0.f) {
        const float c = a.max_norm / (sqrtf(*sqnorm) * a.grad_scale + 1e-6f);
        coef *= c < 1.f ? c : 1.f;
    }
    const float step = a.lr / a.bc1;
    const float keep = 1.f - a.lr * a.weight_decay;  // (read by the decoupled form only)
    const long stride = (long)gridDim.x * 256 * 4;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (lazy_skip(z, i)) continue;
        if (i + 3 < n) {
            float4 pp = *reinterpret_cast<float4*>(p + i);
            const float4 gg = *reinterpret_cast<const float4*>(g + i);
            float4 mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
            float pe[4] = {pp.x, pp.y, pp.z, pp.w}, ge[4] = {gg.x, gg.y, gg.z, gg.w};
            float me[4] = {mm.x, mm.y, mm.z, mm.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float gr;
                if constexpr (DECOUPLED) gr = ge[e] * coef;
                else gr = ge[e] * coef + a.weight_decay * pe[e];
                me[e] = a.beta1 * me[e] + (1.f - a.beta1) * gr;
                ve[e] = a.beta2 * ve[e] + (1.f - a.beta2) * gr * gr;
                if constexpr (DECOUPLED) pe[e] = pe[e] * keep - step * me[e] / (sqrtf(ve[e]) / a.bc2_sqrt + a.eps);
                else pe[e] -= step * me[e] / (sqrtf(ve[e]) / a.bc2_sqrt + a.eps);
            }
            *reinterpret_cast<float4*>(p + i) = make_float4(pe[0], pe[1], pe[2], pe[3]);
            *reinterpret_cast<float4*>(m + i) = make_float4(me[0], me[1], me[2], me[3]);
            *reinterpret_cast<float4*>(v + i) = make_float4(ve[0], ve[1], ve[2], ve[3]);
            if (shadow) *reinterpret_cast<uint2*>(shadow + i) = make_uint2(pack_bf2(pe[0], pe[1]), pack_bf2(pe[2], pe[3]));
        } else {
            for (long k = i; k < n; ++k) {
                float gr, pk;
                if constexpr (DECOUPLED) gr = g[k] * coef;
                else gr = g[k] * coef + a.weight_decay * p[k];
                float mk = a.beta1 * m[k] + (1.f - a.beta1) * gr;
                float vk = a.beta2 * v[k] + (1.f - a.beta2) * gr * gr;
                if constexpr (DECOUPLED) pk = p[k] * keep - step * mk / (sqrtf(vk) / a.bc2_sqrt + a.eps);
                else pk = p[k] - step * mk / (sqrtf(vk) / a.bc2_sqrt + a.eps);
                p[k] = pk, m[k] = mk, v[k] = vk;
                if (shadow) shadow[k] = f2bf(pk);
            }
        }
    }
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n) {
    const long stride = (long)gridDim.x * 256 * 4;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            *reinterpret_cast<uint2*>(y + i) = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
        } else {
            for (long k = i; k < n; ++k) y[k] = f2bf(x[k]);
        }
    }
}

static int grid_for(long n) {
    long b = (n + 1023) / 1024;
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

extern "C" int mmvid_grad_sqnorm(const float* g, int64_t n, float* out_accum, void* stream) {
    MMVID_REQUIRE(g && out_accum && n >= 0, "grad_sqnorm: bad arguments");
    MMVID_REQUIRE(((uintptr_t)g & 15) == 0, "grad_sqnorm: buffer must be 16-byte aligned");
    if (n == 0) return MMVID_OK;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, (long)n, out_accum);
    MMVID_LAUNCH_CHECK("grad_sqnorm");
    return MMVID_OK;
}

// fixed-order version of grad_sqnorm: per-block partial sums, then one block adds them in index order (deterministic:
// the clip coefficient of a step no longer depends on atomic arrival order)
__global__ __launch_bounds__(256) void grad_sqnorm_partial_kernel(const float* __restrict__ g, long n, float* __restrict__ part,
                                                                  LazyRows z) {
    float a = 0.f;
    const long stride = (long)gridDim.x * 256 * 4;
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (lazy_skip(z, i)) continue;
        if (i + 3 < n) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            a += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        } else {
            for (long k = i; k < n; ++k) a += g[k] * g[k];
        }
    }
    a = wave_sum(a);
    __shared__ float sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ float sh[256];
    float a = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) a += part[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] += sh[0];
}

extern "C" int mmvid_grad_sqnorm_det(const float* g, int64_t n, float* partials, float* out_accum, void* stream) {
    return mmvid_grad_sqnorm_rows(g, n, partials, out_accum, nullptr, 0, 0, 0, stream);
}

extern "C" int mmvid_grad_sqnorm_rows(const float* g, int64_t n, float* partials, float* out_accum, const uint8_t* row_flags,
                                      int64_t table_lo, int64_t table_rows, int rowlen, void* stream) {
    MMVID_REQUIRE(g && partials && out_accum && n >= 0, "grad_sqnorm_det: bad arguments");
    MMVID_REQUIRE(((uintptr_t)g & 15) == 0, "grad_sqnorm_det: buffer must be 16-byte aligned");
    LazyRows z;
    if (int rc = make_lazy(z, "grad_sqnorm_det", row_flags, table_lo, table_rows, rowlen, n)) return rc;
    if (n == 0) return MMVID_OK;
    const int nb = grid_for(n);  // <= 2048: `partials` holds 2048 floats
    hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, g, (long)n, partials, z);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nb, out_accum);
    MMVID_LAUNCH_CHECK("grad_sqnorm_det");
    return MMVID_OK;
}

// every Adam entry (no device learning rate, no table, skip_dev NULL where it takes none): one set of checks, one kernel in the
// form the entry names (DECOUPLED false: every entry but mmvid_adam_step_decoupled)
template <bool DECOUPLED>
static int adam_launch(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, const float* lr_dev,
                       float beta1, float beta2, float eps, float weight_decay, int step, const float* step_dev, float max_norm,
                       const float* sqnorm, float grad_scale, const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen,
                       const int32_t* skip_dev, void* stream) {
    MMVID_REQUIRE(p && g && m && v && n >= 0 && (step >= 1 || step_dev), "adam_step: bad arguments");
    MMVID_REQUIRE(!row_flags || weight_decay == 0.f, "adam_step: lazy rows are exact only without weight decay");
    LazyRows z;
    if (int rc = make_lazy(z, "adam_step", row_flags, table_lo, table_rows, rowlen, n)) return rc;
    MMVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && ((uintptr_t)shadow_bf16 & 7) == 0,
                  "adam_step: buffers must be 16-byte aligned");
    if (n == 0) return MMVID_OK;
    AdamArgs a;
    a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.weight_decay = weight_decay;
    const BiasCorrections bc = bias_corrections(beta1, beta2, (float)(step >= 1 ? step : 1));
    a.bc1 = bc.bc1, a.bc2_sqrt = bc.bc2_sqrt;
    a.max_norm = max_norm, a.grad_scale = grad_scale;
    hipLaunchKernelGGL(adam_kernel<DECOUPLED>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)shadow_bf16,
                       (long)n, a, sqnorm, step_dev, lr_dev, z, (const int*)skip_dev);
    MMVID_LAUNCH_CHECK("adam_step");
    return MMVID_OK;
}

extern "C" int mmvid_adam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int step,
                               const float* step_dev, float max_norm, const float* sqnorm, float grad_scale,
                               void* stream) {
    return adam_launch<false>(p, g, m, v, shadow_bf16, n, lr, nullptr, beta1, beta2, eps, weight_decay, step, step_dev, max_norm, sqnorm,
                       grad_scale, nullptr, 0, 0, 0, nullptr, stream);
}

extern "C" int mmvid_adam_step_lr(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                                  const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                                  const float* step_dev, float max_norm, const float* sqnorm, float grad_scale, void* stream) {
    return adam_launch<false>(p, g, m, v, shadow_bf16, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step, step_dev, max_norm, sqnorm,
                       grad_scale, nullptr, 0, 0, 0, nullptr, stream);
}

extern "C" int mmvid_adam_step_rows(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                                    const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                                    const float* step_dev, float max_norm, const float* sqnorm, float grad_scale,
                                    const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen, void* stream) {
    return adam_launch<false>(p, g, m, v, shadow_bf16, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step, step_dev, max_norm, sqnorm,
                       grad_scale, row_flags, table_lo, table_rows, rowlen, nullptr, stream);
}

extern "C" int mmvid_adam_step_guarded(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                                       const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                                       const float* step_dev, float max_norm, const float* sqnorm, float grad_scale,
                                       const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen,
                                       const int32_t* skip_dev, void* stream) {
    MMVID_REQUIRE(((uintptr_t)skip_dev & 3) == 0, "adam_step_guarded: skip_dev must be 4-byte aligned");
    return adam_launch<false>(p, g, m, v, shadow_bf16, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step, step_dev, max_norm, sqnorm,
                       grad_scale, row_flags, table_lo, table_rows, rowlen, skip_dev, stream);
}

extern "C" int mmvid_adam_step_decoupled(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr,
                                         const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int step,
                                         const float* step_dev, float max_norm, const float* sqnorm, float grad_scale,
                                         const uint8_t* row_flags, int64_t table_lo, int64_t table_rows, int rowlen,
                                         const int32_t* skip_dev, void* stream) {
    MMVID_REQUIRE(((uintptr_t)skip_dev & 3) == 0, "adam_step_decoupled: skip_dev must be 4-byte aligned");
    // (also false for NaN.  A row that never saw a gradient still decays: adam_launch refuses a table with weight_decay != 0)
    MMVID_REQUIRE(weight_decay >= 0.f && weight_decay <= 3.0e38f, "adam_step_decoupled: weight_decay must be finite and >= 0");
    return adam_launch<true>(p, g, m, v, shadow_bf16, n, lr, lr_dev, beta1, beta2, eps, weight_decay, step, step_dev, max_norm, sqnorm,
                             grad_scale, row_flags, table_lo, table_rows, rowlen, skip_dev, stream);
}

// The verdict of the non-finite guard and its counters (include/mmvid_hip_ext.h states the rule; tests/guard_ref.py is the host
// replica).  One thread, plain loads and stores: the kernels that follow on the stream read guard_i[0].
__global__ void step_guard_kernel(const float* __restrict__ sqnorm, float grad_scale, float* __restrict__ step_dev,
                                  int* __restrict__ guard_i, float* __restrict__ guard_f) {
    const float sq = *sqnorm;
    const int skip = !finite_bits(sq);  // inf or NaN
    const float norm = __fmul_rn(sqrtf(sq), grad_scale);                 // what adam_kernel clips on
    guard_i[0] = skip;
    guard_i[1] += skip;
    guard_i[2] = skip ? guard_i[2] + 1 : 0;
    guard_i[3] += 1;
    guard_f[0] = norm;
    if (!skip) {
        guard_f[1] = norm;
        *step_dev += 1.f;
    }
}

extern "C" int mmvid_step_guard(const float* sqnorm, float grad_scale, float* step_dev, int32_t* guard_i, float* guard_f,
                                void* stream) {
    MMVID_REQUIRE(sqnorm && step_dev && guard_i && guard_f, "step_guard: sqnorm, step_dev, guard_i and guard_f must not be NULL");
    MMVID_REQUIRE((((uintptr_t)sqnorm | (uintptr_t)step_dev | (uintptr_t)guard_i | (uintptr_t)guard_f) & 3) == 0,
                  "step_guard: pointers must be 4-byte aligned");
    hipLaunchKernelGGL(step_guard_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sqnorm, grad_scale, step_dev, (int*)guard_i,
                       guard_f);
    MMVID_LAUNCH_CHECK("step_guard");
    return MMVID_OK;
}

// The closed-form schedules of mmvid_lr_schedule_ext (include/mmvid_hip_ext.h states the rules; tests/sched_ref.py is the host
// replica).  One thread; ns = scheduler steps taken before this iteration (train.py:373-374).  Every product, sum and quotient is
// one rounded fp32 operation (no contraction: the intrinsics), so the replica's count of roundings is the kernel's.
__global__ void lr_schedule_ext_kernel(const float* __restrict__ step_dev, int kind, float lr_min, float lr_max, long every, long a,
                                       long b, float gamma, float* __restrict__ lr_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long ns = (long)step_dev[0] / every;
    float lr = lr_max;
    if (kind == 2) {  // StepLR
        lr = __fmul_rn(lr_max, powf(gamma, (float)(ns / a)));
    } else if (kind == 3) {  // CosineAnnealingLR: the argument reduced in integers, r in [0, 2a)
        const long r = ns % (2 * a);
        const float x = __fdiv_rn(__fmul_rn(3.14159265358979323846f, (float)r), (float)a);
        lr = __fadd_rn(lr_min, __fmul_rn(__fmul_rn(__fsub_rn(lr_max, lr_min), __fadd_rn(1.f, cosf(x))), 0.5f));
    } else if (ns > 0) {  // kind 4, WarmupDecayLR
        const long k = ns - 1, wu = warmup_clamped(a), span = b - wu > 1 ? b - wu : 1;
        const float g = k < wu ? warmup_log_gamma(k, wu) : fmaxf(0.f, __fdiv_rn((float)(b - k), (float)span));
        lr = __fadd_rn(lr_min, __fmul_rn(__fsub_rn(lr_max, lr_min), g));
    }
    lr_out[0] = lr;
}

extern "C" int mmvid_lr_schedule_ext(const float* step_dev, int kind, float lr_min, float lr_max, int every, int64_t a, int64_t b,
                                     float gamma, float* lr_out, void* stream) {
    MMVID_REQUIRE(step_dev && lr_out, "lr_schedule_ext: null pointer");
    MMVID_REQUIRE((((uintptr_t)step_dev | (uintptr_t)lr_out) & 3) == 0, "lr_schedule_ext: pointers must be 4-byte aligned");
    MMVID_REQUIRE(kind >= 2 && kind <= 4, "lr_schedule_ext: kind %d (2 StepLR, 3 CosineAnnealingLR, 4 WarmupDecayLR; 0 and 1 are "
                                          "mmvid_lr_schedule's)", kind);
    MMVID_REQUIRE(every >= 1, "lr_schedule_ext: every = %d must be >= 1", every);
    // (above 2^24 = where the fp32 step count stops: no iteration reaches such a period, and below it every int -> float is exact)
    MMVID_REQUIRE(a >= 1 && a <= (1L << 24), "lr_schedule_ext: a = %lld outside [1, 2^24]", (long long)a);
    if (kind == 4)
        MMVID_REQUIRE(b >= a && b <= (1L << 24), "lr_schedule_ext: total steps b = %lld outside [a = %lld, 2^24]", (long long)b,
                      (long long)a);
    if (kind == 2) MMVID_REQUIRE(gamma > 0.f && gamma <= 1.f, "lr_schedule_ext: gamma = %g outside (0, 1]", (double)gamma);
    hipLaunchKernelGGL(lr_schedule_ext_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_dev, kind, lr_min, lr_max, (long)every,
                       (long)a, (long)b, gamma, lr_out);
    MMVID_LAUNCH_CHECK("lr_schedule_ext");
    return MMVID_OK;
}

// ReduceLROnPlateau(mode='min', threshold_mode='rel') as one device thread (include/mmvid_hip_ext.h states the rule;
// tests/sched_ref.py is the host replica, bit for bit: multiplies, subtractions and comparisons only, none contracted).
__global__ void lr_plateau_kernel(const float* __restrict__ loss_dev, const float* __restrict__ step_dev, long every, float factor,
                                  int patience, int cooldown, float threshold, float min_lr, float eps, float* __restrict__ state_f,
                                  int* __restrict__ state_i, const int* __restrict__ skip) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (step_skipped(skip) || (long)step_dev[0] % every != 0) return;
    const float loss = loss_dev[0];
    float lr = state_f[0], best = state_f[1];
    int bad = state_i[0], cool = state_i[1], reductions = state_i[2];
    if (loss < __fmul_rn(best, __fsub_rn(1.f, threshold))) best = loss, bad = 0;  // (NaN compares false: a bad epoch)
    else bad += 1;
    if (cool > 0) cool -= 1, bad = 0;
    if (bad > patience) {
        const float nw = fmaxf(__fmul_rn(lr, factor), min_lr);
        if (__fsub_rn(lr, nw) > eps) lr = nw, reductions += 1;
        cool = cooldown, bad = 0;
    }
    state_f[0] = lr, state_f[1] = best;
    state_i[0] = bad, state_i[1] = cool, state_i[2] = reductions;
}

extern "C" int mmvid_lr_plateau(const float* loss_dev, const float* step_dev, int every, float factor, int patience, int cooldown,
                                float threshold, float min_lr, float eps, float* state_f, int32_t* state_i, const int32_t* skip_dev,
                                void* stream) {
    MMVID_REQUIRE(loss_dev && step_dev && state_f && state_i, "lr_plateau: loss_dev, step_dev, state_f and state_i must not be NULL");
    MMVID_REQUIRE((((uintptr_t)loss_dev | (uintptr_t)step_dev | (uintptr_t)state_f | (uintptr_t)state_i | (uintptr_t)skip_dev) & 3) == 0,
                  "lr_plateau: pointers must be 4-byte aligned");
    MMVID_REQUIRE(every >= 1, "lr_plateau: every = %d must be >= 1", every);
    MMVID_REQUIRE(factor > 0.f && factor < 1.f, "lr_plateau: factor = %g outside (0, 1)", (double)factor);
    MMVID_REQUIRE(patience >= 0 && cooldown >= 0, "lr_plateau: patience = %d and cooldown = %d must be >= 0", patience, cooldown);
    MMVID_REQUIRE(threshold >= 0.f && threshold < 1.f && min_lr >= 0.f && min_lr <= 3.0e38f && eps >= 0.f && eps <= 3.0e38f,
                  "lr_plateau: threshold in [0, 1), min_lr and eps finite and >= 0");
    hipLaunchKernelGGL(lr_plateau_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss_dev, step_dev, (long)every, factor, patience,
                       cooldown, threshold, min_lr, eps, state_f, (int*)state_i, (const int*)skip_dev);
    MMVID_LAUNCH_CHECK("lr_plateau");
    return MMVID_OK;
}

extern "C" int mmvid_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream) {
    MMVID_REQUIRE(x && y && n >= 0, "cast_f32_to_bf16: bad arguments");
    MMVID_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0, "cast_f32_to_bf16: alignment");
    if (n == 0) return MMVID_OK;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, (long)n);
    MMVID_LAUNCH_CHECK("cast_f32_to_bf16");
    return MMVID_OK;
}
