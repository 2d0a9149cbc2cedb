// Native executor for the VQGAN encoder / decoder op sequence (taming Encoder/Decoder.forward,
// model.py:439-466, 551-582; vae.py:38-56).  The host builds the op list once per input shape
// (mmvid_amd/vqgan_plan.py) -- convs, GroupNorm+swish, casts, spatial attention, VQ lookup, codebook gather, layout
// kernels, all on offsets into one arena -- and each call is then a single host->native transition that
// enqueues ~190 kernels back to back (the Python-per-op version was host-bound: 12 ms of launch overhead for
// 8.5 ms of GPU work per 48-frame encode).  No allocation, no sync: graph-capturable.
// mmvid_vqgan_check says what a well-formed list is (the table in include/mmvid_hip.h) and mmvid_vqgan_run asks it first, so the
// enqueue_*_op functions see accepted records only and test a flag exactly where two accepted records differ.
#include "../../include/mmvid_hip.h"
#include "common.h"
#include "graphs.h"

namespace {
enum {
    RES_F32 = MMVID_VQFLAG_RES_F32, IN_F32 = MMVID_VQFLAG_IN_F32, CLAMP01 = MMVID_VQFLAG_CLAMP01, STATS_GIVEN = MMVID_VQFLAG_STATS_GIVEN,
    EMIT_STATS = MMVID_VQFLAG_EMIT_STATS, STRIP = MMVID_VQFLAG_STRIP, BLOCKS64 = MMVID_VQFLAG_BLOCKS64, STRICT = MMVID_VQFLAG_STRICT,
    SPLITK = MMVID_VQFLAG_SPLITK, SPLIT = MMVID_VQFLAG_SPLIT, F16 = MMVID_VQFLAG_F16
};
typedef mmvid_vqgan_op_t op_t;

// ---- the checker ---------------------------------------------------------------------------------------------------------------------
enum { BF16_OPERATOR, PAIR_OPERATOR, STRICT_OPERATOR };
// the flags an operator takes besides STRICT / SPLIT: {on a CONV, on a GROUPNORM}; none on any other op
const int LEGAL[3][2] = {{RES_F32 | CLAMP01 | EMIT_STATS | STRIP | SPLITK, IN_F32 | STATS_GIVEN | BLOCKS64},
                         {CLAMP01 | EMIT_STATS | STRIP | SPLITK | F16, STATS_GIVEN | BLOCKS64 | F16},
                         {CLAMP01, 0}};
constexpr int bit(int op) { return 1 << op; }
const int HAS_OP[3] = {bit(MMVID_VQOP_EXT_CAST + 1) - 1,  // all nine
                       bit(MMVID_VQOP_IMG2NHWC8) | bit(MMVID_VQOP_CONV) | bit(MMVID_VQOP_GROUPNORM) | bit(MMVID_VQOP_CAST),
                       bit(MMVID_VQOP_IMG2NHWC8) | bit(MMVID_VQOP_CONV) | bit(MMVID_VQOP_GROUPNORM) | bit(MMVID_VQOP_SPATIAL_ATTN) |
                           bit(MMVID_VQOP_GATHER) | bit(MMVID_VQOP_EXT_CAST)};

const char* flag_name(int flag, bool groupnorm) {
    switch (flag) {
        case 1: return groupnorm ? "IN_F32" : "RES_F32";
        case 2: return groupnorm ? "STATS_GIVEN" : "CLAMP01";
        case 4: return "EMIT_STATS";
        case 8: return groupnorm ? "BLOCKS64" : "STRIP";
        case 32: return "SPLITK";
        case 128: return "F16";
        default: return "a bit without a name";
    }
}

// nullptr, or what is wrong with the record: the flags by name and the rule.  *bad_flag: set instead when the rule is "this flag is not
// in the table for this operator and op"
const char* refusal(const op_t& o, int* bad_flag) {
    const int f = o.flags;
    if ((f & STRICT) && (f & SPLIT)) return "STRICT with SPLIT: a record belongs to one operator";
    if (o.op < 0 || o.op > MMVID_VQOP_EXT_CAST) return "unknown op code";
    const int k = (f & STRICT) ? STRICT_OPERATOR : ((f & SPLIT) ? PAIR_OPERATOR : BF16_OPERATOR);
    if (!(HAS_OP[k] & bit(o.op))) return k == STRICT_OPERATOR ? "STRICT: the op has no strict form" : "SPLIT: the op has no split form";
    const bool conv = o.op == MMVID_VQOP_CONV, gn = o.op == MMVID_VQOP_GROUPNORM;
    const int extra = f & ~(STRICT | SPLIT) & ~((conv || gn) ? LEGAL[k][gn] : 0);
    if (extra) {
        *bad_flag = extra & -extra;
        return nullptr;
    }
    if (conv) {
        if ((f & EMIT_STATS) && (f & SPLITK)) return "EMIT_STATS with SPLITK: both use `scratch`";
        if ((f & EMIT_STATS) && o.scratch < 0) return "EMIT_STATS without a stats area at `scratch`";
        if ((f & SPLITK) && o.scratch < 0) return "SPLITK without a workspace at `scratch`";
        if ((f & STRIP) && (f & CLAMP01)) return "STRIP with CLAMP01: the strip kernel has no such epilogue";
        if ((f & STRIP) && (f & SPLITK)) return "STRIP with SPLITK";
        if ((f & STRIP) && o.mode != 0) return "STRIP with mode != 0: the strip kernel is 3x3 stride 1";
        if ((f & F16) && !(f & STRIP)) return "F16 without STRIP: only the strip kernel reads an fp16 plane";
        if ((f & RES_F32) && o.in1 < 0) return "RES_F32 without a residual at in1";
        if (o.out_bf16 < 0 && o.out_f32 < 0) return "neither out_bf16 nor out_f32 is given";
    }
    if (gn) {
        if ((f & BLOCKS64) && !(f & STATS_GIVEN)) return "BLOCKS64 without STATS_GIVEN";
        if (o.scratch < 0) return "GROUPNORM without a stats area at `scratch`";
    }
    return nullptr;
}

// ---- the walk: what the enqueue functions share ---------------------------------------------------------------------------------------
inline char* at(void* arena, int64_t off) { return off < 0 ? nullptr : (char*)arena + off; }
inline int64_t elements(const op_t& o) { return (int64_t)o.N * o.H * o.W * o.C; }
// CONV with EMIT_STATS: where the epilogue writes the partial sums of its output, in the stats area at `scratch`
inline float* emitted_partials(void* arena, const op_t& o) {
    return (o.flags & EMIT_STATS) ? gn_stats_partials((float*)at(arena, o.scratch), o.N, o.Cout) : nullptr;
}
// GROUPNORM: how many partial blocks per image the producing CONV wrote (0: a statistics pass runs in the GroupNorm)
inline int partial_blocks(const op_t& o) { return (o.flags & STATS_GIVEN) ? (o.H * o.W) / ((o.flags & BLOCKS64) ? 64 : 128) : 0; }
// bf16 CONV: the residual at in1, as the (bf16, fp32) pair of pointers the convolutions take
inline const void* residual_bf16(void* arena, const op_t& o) { return (o.flags & RES_F32) ? nullptr : at(arena, o.in1); }
inline const float* residual_f32(void* arena, const op_t& o) { return (o.flags & RES_F32) ? (const float*)at(arena, o.in1) : nullptr; }

// the fp32-accurate operator (strict.hip): every arena tensor of the plan is fp32
int enqueue_strict_op(const op_t& o, void* arena, void* stream) {
    switch (o.op) {
        case MMVID_VQOP_IMG2NHWC8:
            return mmvid_image_to_nhwc4_f32((const float*)o.ext_in, o.N, o.H, o.W, (float*)at(arena, o.out_f32), stream);
        case MMVID_VQOP_CONV:
            return mmvid_conv2d_nhwc_f32(o.mode, (const float*)at(arena, o.in0), o.N, o.H, o.W, o.C, (const float*)o.w, o.b, o.Cout,
                                         (const float*)at(arena, o.in1), (o.flags & CLAMP01) != 0, (float*)at(arena, o.out_f32), stream);
        case MMVID_VQOP_GROUPNORM:
            return mmvid_groupnorm_swish_nhwc_f32((const float*)at(arena, o.in0), o.N, (int64_t)o.H * o.W, o.C, (const float*)o.w, o.b,
                                                  o.eps, o.mode, (float*)at(arena, o.scratch), (float*)at(arena, o.out_f32), stream);
        case MMVID_VQOP_SPATIAL_ATTN:
            return mmvid_spatial_attention_f32((const float*)at(arena, o.in0), (const float*)at(arena, o.in1),
                                               (const float*)at(arena, o.in2), o.N, o.H * o.W, o.C, o.eps, (float*)at(arena, o.scratch),
                                               (float*)at(arena, o.out_f32), stream);
        case MMVID_VQOP_GATHER:
            return mmvid_gather_rows((const float*)o.w, o.Cout, (const int64_t*)o.ext_in, (int64_t)o.N * o.H * o.W, o.C,
                                     (float*)at(arena, o.out_f32), nullptr, stream);
        default:  // MMVID_VQOP_EXT_CAST
            if (hipMemcpyAsync(at(arena, o.out_f32), o.ext_in, (size_t)elements(o) * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
                hipSuccess) {
                mmvid_set_error("vqgan_run: memcpy failed");
                return MMVID_ERR_HIP;
            }
            return MMVID_OK;
    }
}

// the bf16-pair operator (conv.hip: mmvid_conv2d_nhwc_split3); F16: one fp16 product on the fp16 plane a GROUPNORM with F16 wrote
int enqueue_pair_op(const op_t& o, void* arena, void* stream) {
    switch (o.op) {
        case MMVID_VQOP_IMG2NHWC8:
            return mmvid_image_to_nhwc8_split((const float*)o.ext_in, o.N, o.H, o.W, at(arena, o.out_bf16), stream);
        case MMVID_VQOP_CONV:
            if (o.flags & STRIP)
                return ((o.flags & F16) ? mmvid_conv3x3_strip_nhwc_f16 : mmvid_conv3x3_strip_nhwc_split3)(
                    at(arena, o.in0), o.N, o.H, o.W, o.C, o.w, o.b, o.Cout, (const float*)at(arena, o.in1), (float*)at(arena, o.out_f32),
                    emitted_partials(arena, o), at(arena, o.out_bf16), stream);
            return mmvid_conv2d_nhwc_split3(o.mode, at(arena, o.in0), o.N, o.H, o.W, o.C, o.w, o.b, o.Cout, (const float*)at(arena, o.in1),
                                            (o.flags & CLAMP01) != 0, (float*)at(arena, o.out_f32), emitted_partials(arena, o),
                                            (o.flags & SPLITK) ? 4 : 1, (o.flags & SPLITK) ? (float*)at(arena, o.scratch) : nullptr, stream);
        case MMVID_VQOP_GROUPNORM:
            return ((o.flags & F16) ? mmvid_groupnorm_swish_nhwc_f16out : mmvid_groupnorm_swish_nhwc_split)(
                (const float*)at(arena, o.in0), o.N, (int64_t)o.H * o.W, o.C, (const float*)o.w, o.b, o.eps, o.mode,
                (float*)at(arena, o.scratch), partial_blocks(o), at(arena, o.out_bf16), stream);
        default:  // MMVID_VQOP_CAST
            return mmvid_split_f32_bf16x2((const float*)at(arena, o.in0), elements(o), at(arena, o.out_bf16), stream);
    }
}

int enqueue_bf16_op(const op_t& o, void* arena, void* stream) {
    switch (o.op) {
        case MMVID_VQOP_IMG2NHWC8:
            return mmvid_image_to_nhwc8((const float*)o.ext_in, o.N, o.H, o.W, at(arena, o.out_bf16), stream);
        case MMVID_VQOP_CONV:
            if (o.flags & STRIP)  // 3x3 stride-1 convolution in strip form (the planner checked the geometry)
                return mmvid_conv3x3_strip_nhwc(at(arena, o.in0), o.N, o.H, o.W, o.C, o.w, o.b, o.Cout, residual_bf16(arena, o),
                                                residual_f32(arena, o), at(arena, o.out_bf16), (float*)at(arena, o.out_f32),
                                                emitted_partials(arena, o), stream);
            // SPLITK: a deep layer on a small map, split-K by 4 with a fixed-order reduce
            return mmvid_conv2d_nhwc_splitk(o.mode, at(arena, o.in0), o.N, o.H, o.W, o.C, o.w, o.b, o.Cout, residual_bf16(arena, o),
                                            residual_f32(arena, o), (o.flags & CLAMP01) != 0, at(arena, o.out_bf16),
                                            (float*)at(arena, o.out_f32), emitted_partials(arena, o), (o.flags & SPLITK) ? 4 : 1,
                                            (o.flags & SPLITK) ? (float*)at(arena, o.scratch) : nullptr, stream);
        case MMVID_VQOP_GROUPNORM:
            return mmvid_groupnorm_swish_nhwc(at(arena, o.in0), (o.flags & IN_F32) ? 0 : 1, o.N, (int64_t)o.H * o.W, o.C,
                                              (const float*)o.w, o.b, o.eps, o.mode, (float*)at(arena, o.scratch), partial_blocks(o),
                                              at(arena, o.out_bf16), (float*)at(arena, o.out_f32), stream);
        case MMVID_VQOP_CAST:
            return mmvid_cast_f32_to_bf16((const float*)at(arena, o.in0), at(arena, o.out_bf16), elements(o), stream);
        case MMVID_VQOP_SPATIAL_ATTN:
            return mmvid_spatial_attention_ld(at(arena, o.in0), at(arena, o.in1), at(arena, o.in2), o.pad > 0 ? o.pad : o.C, o.N,
                                              o.H * o.W, o.C, o.eps, (float*)at(arena, o.scratch), at(arena, o.out_bf16), stream);
        case MMVID_VQOP_VQ_ARGMIN:
            return mmvid_vq_argmin_l2((const float*)at(arena, o.in0), (const float*)o.w, o.b, (int64_t)o.N * o.H * o.W, o.Cout, o.C,
                                      (int64_t*)o.ext_out, nullptr, stream);
        case MMVID_VQOP_GATHER:
            return mmvid_gather_rows((const float*)o.w, o.Cout, (const int64_t*)o.ext_in, (int64_t)o.N * o.H * o.W, o.C, nullptr,
                                     at(arena, o.out_bf16), stream);
        case MMVID_VQOP_EXT_CAST:
            return mmvid_cast_f32_to_bf16((const float*)o.ext_in, at(arena, o.out_bf16), elements(o), stream);
        default:  // MMVID_VQOP_NHWC2NCHW
            return mmvid_nhwc_to_nchw_f32((const float*)at(arena, o.in0), o.N, o.H, o.W, o.C, o.Cout, (float*)o.ext_out, stream);
    }
}

int vqgan_enqueue(const op_t* ops, int nops, void* arena, void* stream) {
    for (int i = 0; i < nops; ++i) {
        const op_t& o = ops[i];
        const int rc = (o.flags & STRICT) ? enqueue_strict_op(o, arena, stream)
                                          : ((o.flags & SPLIT) ? enqueue_pair_op(o, arena, stream) : enqueue_bf16_op(o, arena, stream));
        if (rc) return rc;
    }
    return MMVID_OK;
}
}  // namespace

extern "C" int mmvid_vqgan_check(const mmvid_vqgan_op_t* ops, int nops) {
    MMVID_REQUIRE(nops >= 0 && (ops || nops == 0), "vqgan_check: bad arguments");
    for (int i = 0; i < nops; ++i) {
        int bad_flag = 0;
        const char* why = refusal(ops[i], &bad_flag);
        if (bad_flag)
            mmvid_set_error("vqgan_check: op %d (code %d, flags %d): %s is not a flag of this op under its operator", i, ops[i].op,
                            ops[i].flags, flag_name(bad_flag, ops[i].op == MMVID_VQOP_GROUPNORM));
        else if (why)
            mmvid_set_error("vqgan_check: op %d (code %d, flags %d): %s", i, ops[i].op, ops[i].flags, why);
        if (bad_flag || why) return MMVID_ERR_ARG;
    }
    return MMVID_OK;
}

extern "C" int mmvid_vqgan_run(const mmvid_vqgan_op_t* ops, int nops, void* arena, void* stream) {
    MMVID_REQUIRE(ops && arena && nops >= 0, "vqgan_run: bad arguments");
    if (int rc = mmvid_vqgan_check(ops, nops)) return rc;  // before anything is enqueued
    uint64_t key = mmvid_hash_bytes(ops, sizeof(mmvid_vqgan_op_t) * (size_t)nops, 0xcbf29ce484222325ull ^ 1);
    key = mmvid_hash_ptr(arena, mmvid_hash_ptr(stream, key));
    return mmvid_run_cached(key, (hipStream_t)stream, [=](hipStream_t s) { return vqgan_enqueue(ops, nops, arena, (void*)s); });
}
