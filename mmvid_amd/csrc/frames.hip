// Output side of sampling: decoded frames to the bytes a GIF / Motion-JPEG writer takes, on the device.
//   utils/utils_html.py:157-186 (save_image): tensor.cpu().clamp(0, 1) * 255 -> uint8 -> permute to [H, W, 3]
// The VQGAN decoder delivers [N, 3, H, W] fp32; a long video (mmvid_amd/long_video.py) would otherwise ship four times the bytes
// to the host and quantise them there on one thread.  One elementwise pass, HBM-bound: 12 bytes read and 3 written per pixel.
#include "../../include/mmvid_hip.h"
#include "common.h"

namespace {

// The reference's arithmetic, one operation at a time: clamp (NaN -> 0: fmaxf returns its other operand), ONE fp32 multiply (no
// fma can form: nothing is added), conversion by truncation.  The product lies in [0, 255], so the unsigned conversion is exact.
__device__ __forceinline__ uint32_t unit_to_u8(float x) {
    const float c = fminf(fmaxf(x, 0.0f), 1.0f);
    return (uint32_t)__fmul_rn(c, 255.0f);
}

struct U3 {
    uint32_t a, b, c;
};

// img [N, 3, HW] fp32 -> out [N, HW, 3] uint8, HW % 4 == 0.  A thread converts 4 pixels: one 16-byte load per channel plane (a wave
// reads three 1 KiB runs) and 12 packed bytes out (a wave writes 768 contiguous bytes).  Grid-stride over the N * HW / 4 groups.
// PASTE (video completion): a group whose token is given copies its 12 bytes from real [N, HW, 3] instead and never loads img;
// given [N, h, w], a token covers ph x pw pixels with pw % 4 == 0, so the 4 pixels of a group share one token.
template <bool PASTE>
__global__ __launch_bounds__(256) void frames_to_u8_kernel(const float* __restrict__ img, long N, long HW, const unsigned char* __restrict__ real,
                                                           const unsigned char* __restrict__ given, int W, int ph, int pw, int h, int w,
                                                           unsigned char* __restrict__ out) {
    const long q = HW >> 2, total = N * q;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long n = idx / q, g = idx - n * q;
        if (PASTE) {
            const int p = (int)(4 * g), y = p / W, x = p - y * W;
            if (given[(n * h + y / ph) * w + x / pw]) {
                *reinterpret_cast<U3*>(out + (n * HW + 4 * g) * 3) = *reinterpret_cast<const U3*>(real + (n * HW + 4 * g) * 3);
                continue;
            }
        }
        const float* src = img + n * 3 * HW + 4 * g;
        const float4 r = *reinterpret_cast<const float4*>(src);
        const float4 gr = *reinterpret_cast<const float4*>(src + HW);
        const float4 bl = *reinterpret_cast<const float4*>(src + 2 * HW);
        // bytes in memory order: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian: the first byte is the low one)
        U3 w3;
        w3.a = unit_to_u8(r.x) | (unit_to_u8(gr.x) << 8) | (unit_to_u8(bl.x) << 16) | (unit_to_u8(r.y) << 24);
        w3.b = unit_to_u8(gr.y) | (unit_to_u8(bl.y) << 8) | (unit_to_u8(r.z) << 16) | (unit_to_u8(gr.z) << 24);
        w3.c = unit_to_u8(bl.z) | (unit_to_u8(r.w) << 8) | (unit_to_u8(gr.w) << 16) | (unit_to_u8(bl.w) << 24);
        *reinterpret_cast<U3*>(out + (n * HW + 4 * g) * 3) = w3;
    }
}

unsigned frames_grid(long N, long hw) {
    const long blocks = (N * (hw / 4) + 255) / 256;
    return (unsigned)(blocks < 2048 ? blocks : 2048);
}

}  // namespace

extern "C" int mmvid_frames_to_u8(const float* img, int64_t N, int H, int W, uint8_t* out, void* stream) {
    MMVID_REQUIRE(img && out && N >= 0 && H > 0 && W > 0, "frames_to_u8: bad arguments");
    const long hw = (long)H * W;
    MMVID_REQUIRE(hw % 4 == 0, "frames_to_u8: H * W = %ld is not a multiple of 4", hw);
    MMVID_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 3) == 0,
                  "frames_to_u8: img must be 16-byte aligned and out 4-byte aligned");
    if (N == 0) return MMVID_OK;
    hipLaunchKernelGGL(frames_to_u8_kernel<false>, dim3(frames_grid((long)N, hw)), dim3(256), 0, (hipStream_t)stream, img, (long)N, hw,
                       (const unsigned char*)nullptr, (const unsigned char*)nullptr, W, 1, 1, 1, 1, out);
    MMVID_LAUNCH_CHECK("frames_to_u8");
    return MMVID_OK;
}

extern "C" int mmvid_frames_paste_u8(const float* img, const uint8_t* real, const uint8_t* given, int64_t N, int H, int W, int h, int w,
                                     uint8_t* out, void* stream) {
    MMVID_REQUIRE(img && real && given && out && N >= 0 && H > 0 && W > 0 && h > 0 && w > 0, "frames_paste_u8: bad arguments");
    MMVID_REQUIRE(H % h == 0 && W % w == 0, "frames_paste_u8: the token grid %d x %d does not divide the frame %d x %d (H %% h == 0, W %% w == 0)",
                  h, w, H, W);
    MMVID_REQUIRE((W / w) % 4 == 0, "frames_paste_u8: a token is W / w = %d pixels wide, not a multiple of 4 ((W / w) %% 4 == 0)", W / w);
    const long hw = (long)H * W;
    MMVID_REQUIRE(hw % 4 == 0 && hw <= 0x7fffffffL, "frames_paste_u8: H * W = %ld is not a multiple of 4 (or above 2^31 - 1)", hw);
    MMVID_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)real & 3) == 0 && ((uintptr_t)out & 3) == 0,
                  "frames_paste_u8: img must be 16-byte aligned, real and out 4-byte aligned");
    if (N == 0) return MMVID_OK;
    hipLaunchKernelGGL(frames_to_u8_kernel<true>, dim3(frames_grid((long)N, hw)), dim3(256), 0, (hipStream_t)stream, img, (long)N, hw,
                       (const unsigned char*)real, (const unsigned char*)given, W, H / h, W / w, h, w, out);
    MMVID_LAUNCH_CHECK("frames_paste_u8");
    return MMVID_OK;
}
