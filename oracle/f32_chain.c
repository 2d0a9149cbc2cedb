/* CPU oracle for the fp32 strict operators (mmvid_amd/csrc/strict.hip).  TEST INFRASTRUCTURE (see oracle/__init__.py).
 *
 * strict.hip promises that every matmul / convolution output element is ONE k-ordered fp32 fmaf chain,
 *     acc = 0.0f;  for k = 0 .. K-1:  acc = fmaf(a[k], b[k], acc)
 * (exact product, one rounding per accumulate), whatever the tiling, the batch size or the launch geometry.  These loops
 * restate exactly that promise in plain C, so that a kernel output can be compared BIT FOR BIT.  The epilogue (bias,
 * residual, clamp) is not here: the tests apply it in torch fp32, one rounding per operation.
 *
 * Several outputs are computed side by side only to hide the latency of a serial fmaf; each output is still its own
 * chain in ascending k, so the grouping cannot change a bit.
 *
 * Build: gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC (see oracle/build.py).
 */
#include <math.h>
#include <stdint.h>

#define NB 8 /* chains advanced together */

/* C[m][n] = chain over k of A[m][k] * B(n,k);  A [M][lda];  B row-major [N][ldb] (k contiguous) or k-major [K][ldb]. */
void oracle_chain_gemm(const float *A, int64_t lda, const float *B, int64_t ldb, int b_kmajor, int64_t M, int64_t N,
                       int64_t K, float *C, int64_t ldc) {
    for (int64_t m = 0; m < M; ++m) {
        const float *a = A + m * lda;
        for (int64_t n0 = 0; n0 < N; n0 += NB) {
            const int64_t nb = N - n0 < NB ? N - n0 : NB;
            float acc[NB];
            for (int64_t j = 0; j < nb; ++j) acc[j] = 0.0f;
            if (b_kmajor) {
                for (int64_t k = 0; k < K; ++k)
                    for (int64_t j = 0; j < nb; ++j) acc[j] = fmaf(a[k], B[k * ldb + n0 + j], acc[j]);
            } else {
                for (int64_t k = 0; k < K; ++k)
                    for (int64_t j = 0; j < nb; ++j) acc[j] = fmaf(a[k], B[(n0 + j) * ldb + k], acc[j]);
            }
            for (int64_t j = 0; j < nb; ++j) C[m * ldc + n0 + j] = acc[j];
        }
    }
}

/* The four modes of mmvid_conv2d_nhwc on x [N][H][W][Cin], w [Cout][taps][Cin], out [N][Hout][Wout][Cout]:
 *   0: 3x3, stride 1, pad 1            1: pad (0,1,0,1) then 3x3 stride 2 (H, W even; Hout = H/2)
 *   2: nearest x2 then 3x3 pad 1       3: 1x1
 * k = (ky, kx, ci) ascending.  A tap that falls into the padding is SKIPPED, not fed as a zero: fmaf(0, w, acc) == acc
 * for every finite w, so both forms give the same bits (tests/test_f32_chain_host.py checks that against chain_gemm on
 * the zero-filled im2col matrix).  Only output pixels m in [m_begin, m_end) of the flattened [N*Hout*Wout] are written,
 * so that a caller can spread them over threads. */
void oracle_chain_conv2d_nhwc(int mode, const float *x, int64_t N, int64_t H, int64_t W, int64_t Cin, const float *w,
                              int64_t Cout, float *out, int64_t m_begin, int64_t m_end) {
    const int64_t Hout = mode == 1 ? H / 2 : mode == 2 ? 2 * H : H;
    const int64_t Wout = mode == 1 ? W / 2 : mode == 2 ? 2 * W : W;
    const int taps = mode == 3 ? 1 : 9;
    (void)N;
    for (int64_t m = m_begin; m < m_end; ++m) {
        const int64_t n = m / (Hout * Wout), rem = m - n * Hout * Wout;
        const int64_t oy = rem / Wout, ox = rem - oy * Wout;
        const float *src[9]; /* input pixel of each tap, or null where the tap is padding */
        for (int t = 0; t < taps; ++t) {
            const int64_t ky = t / 3, kx = t - 3 * ky;
            int64_t iy, ix;
            int ok = 1;
            if (mode == 0) {
                iy = oy + ky - 1, ix = ox + kx - 1;
                ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            } else if (mode == 1) {
                iy = 2 * oy + ky, ix = 2 * ox + kx;
                ok = iy < H && ix < W;
            } else if (mode == 2) { /* (uy, ux) is a pixel of the upsampled map, which repeats x[uy/2][ux/2] */
                const int64_t uy = oy + ky - 1, ux = ox + kx - 1;
                ok = uy >= 0 && uy < 2 * H && ux >= 0 && ux < 2 * W;
                iy = uy / 2, ix = ux / 2;
            } else {
                iy = oy, ix = ox;
            }
            src[t] = ok ? x + ((n * H + iy) * W + ix) * Cin : 0;
        }
        for (int64_t c0 = 0; c0 < Cout; c0 += NB) {
            const int64_t nb = Cout - c0 < NB ? Cout - c0 : NB;
            float acc[NB];
            for (int64_t j = 0; j < nb; ++j) acc[j] = 0.0f;
            for (int t = 0; t < taps; ++t) {
                if (!src[t]) continue;
                const float *wt = w + ((int64_t)c0 * taps + t) * Cin;
                for (int64_t ci = 0; ci < Cin; ++ci)
                    for (int64_t j = 0; j < nb; ++j) acc[j] = fmaf(src[t][ci], wt[j * taps * Cin + ci], acc[j]);
            }
            for (int64_t j = 0; j < nb; ++j) out[m * Cout + c0 + j] = acc[j];
        }
    }
}
