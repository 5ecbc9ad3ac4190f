/*
 * Float32 model of the scaled max-log turbo decoder (tests/turbo_scaled_model.py
 * builds it with the host compiler, -ffp-contract=off).
 *
 * It restates the float32 kernel-verification model of oracle/coding_oracle.c
 * (bcjr_f32, or_turbo_decode_f32: metrics normalised to state 0 every step,
 * -1e30 sentinels, gamma = (Ls/2 +- Lp/2) +- La/2, L = max(a + t0) - max(a + t1)
 * with t = beta + gamma) and adds the one multiply of include/lte_phy.h
 * (lte_plan_set_turbo_scale):
 *
 *     le = s * ((lapp - la) - ls)        in float32, s = (float)scale
 *
 * in both half-iterations.  The a-posteriori L is not scaled.  s = 1 skips the
 * multiply (x * 1.0f == x anyway).
 *
 * D(n), the decisions of a decode of n iterations, are the signs of the
 * decoder-1 pass that follows iteration n (the final pass of that decode has
 * the same inputs), so one run of `iters` iterations yields D(0) .. D(iters):
 * out [iters + 1][K].
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline float fmx(float a, float b) { return a > b ? a : (b > a ? b : a); }

/* gamma of (fb, par, u) from c = {g(0,0,0), g(0,0,1), g(0,1,0), g(0,1,1)} */
static inline float gsel(const float c[4], int fb, int par, int u)
{
    return fb == 0 ? c[par * 2 + u] : -c[(1 - par) * 2 + (1 - u)];
}

/* one max-log BCJR pass: n = K + 3 steps, the last three the termination
 * steps (a priori 0, no output); state s = 4 s0 + 2 s1 + s2, next state
 * 4 fb + 2 s0 + s1 with fb = u ^ s1 ^ s2, parity fb ^ s0 ^ s2 */
static void bcjr32(const float *Ls, const float *Lp, const float *La, int n, int K, float *Lapp, float *alpha)
{
    const float NEG = -1.0e30f;
    float a[8], b[8], t0[8], t1[8];
    a[0] = 0.0f;
    for (int s = 1; s < 8; ++s) a[s] = NEG;
    for (int k = 0; k < K; ++k) {
        memcpy(alpha + (size_t)k * 8, a, sizeof a);
        const float hs = 0.5f * Ls[k], hp = 0.5f * Lp[k], ha = 0.5f * La[k];
        const float sp = hs + hp, sm = hs - hp;
        const float c[4] = {sp + ha, sp - ha, sm + ha, sm - ha};
        float o[8];
        for (int ns = 0; ns < 8; ++ns) {
            const int f = ns >> 2, s0 = (ns >> 1) & 1, s1 = ns & 1;
            const float v0 = a[4 * s0 + 2 * s1] + gsel(c, f, f ^ s0, f ^ s1);
            const float v1 = a[4 * s0 + 2 * s1 + 1] + gsel(c, f, f ^ s0 ^ 1, f ^ s1 ^ 1);
            o[ns] = fmx(v0, v1);
        }
        const float n0 = o[0];
        a[0] = 0.0f;
        for (int s = 1; s < 8; ++s) a[s] = o[s] - n0;
    }
    b[0] = 0.0f;
    for (int s = 1; s < 8; ++s) b[s] = NEG;
    for (int k = n - 1; k >= 0; --k) {
        const float la = k < K ? La[k] : 0.0f;
        const float hs = 0.5f * Ls[k], hp = 0.5f * Lp[k], ha = 0.5f * la;
        const float sp = hs + hp, sm = hs - hp;
        const float c[4] = {sp + ha, sp - ha, sm + ha, sm - ha};
        for (int s = 0; s < 8; ++s) {
            const int s0 = s >> 2, s1 = (s >> 1) & 1, s2 = s & 1;
            const int fb = s1 ^ s2, par = fb ^ s0 ^ s2, ns = 4 * fb + 2 * s0 + s1;
            const float g = gsel(c, fb, par, 0);
            t0[s] = b[ns] + g;
            t1[s] = b[ns ^ 4] - g;
        }
        if (k < K) {
            const float *A = alpha + (size_t)k * 8;
            float m0 = A[0] + t0[0], m1 = A[0] + t1[0];
            for (int s = 1; s < 8; ++s) {
                m0 = fmx(m0, A[s] + t0[s]);
                m1 = fmx(m1, A[s] + t1[s]);
            }
            Lapp[k] = m0 - m1;
        }
        for (int s = 0; s < 8; ++s) b[s] = fmx(t0[s], t1[s]);
        const float n0 = b[0];
        b[0] = 0.0f;
        for (int s = 1; s < 8; ++s) b[s] -= n0;
    }
}

/* llr [3K + 12], perm = QPP pi; out [iters + 1][K] = D(0) .. D(iters) */
void tsm_decode_f32(const float *llr, int K, int iters, const int32_t *perm, double scale, uint8_t *out)
{
    const int n = K + 3;
    const float s = (float)scale;
    const int scaled = scale != 1.0;
    float *ls1 = malloc(sizeof(float) * n), *lp1 = malloc(sizeof(float) * n);
    float *ls2 = malloc(sizeof(float) * n), *lp2 = malloc(sizeof(float) * n);
    float *la = malloc(sizeof(float) * n), *lapp = malloc(sizeof(float) * n);
    float *le = calloc(K, sizeof(float)), *alpha = malloc(sizeof(float) * 8 * (size_t)n);
    for (int k = 0; k < K; ++k) {
        ls1[k] = llr[3 * k];
        lp1[k] = llr[3 * k + 1];
        lp2[k] = llr[3 * k + 2];
    }
    for (int t = 0; t < 3; ++t) {
        ls1[K + t] = llr[3 * K + t];
        lp1[K + t] = llr[3 * K + 3 + t];
        ls2[K + t] = llr[3 * K + 6 + t];
        lp2[K + t] = llr[3 * K + 9 + t];
    }
    for (int k = 0; k < K; ++k) ls2[k] = ls1[perm[k]];
    for (int it = 0;; ++it) {
        for (int k = 0; k < K; ++k) la[k] = it == 0 ? 0.0f : le[k];
        bcjr32(ls1, lp1, la, n, K, lapp, alpha);
        for (int k = 0; k < K; ++k) out[(size_t)it * K + k] = lapp[k] < 0.0f ? 1 : 0;
        if (it == iters) break;
        for (int k = 0; k < K; ++k) {
            const float e = (lapp[k] - la[k]) - ls1[k];
            le[k] = scaled ? s * e : e;
        }
        for (int k = 0; k < K; ++k) la[k] = le[perm[k]];
        bcjr32(ls2, lp2, la, n, K, lapp, alpha);
        for (int k = 0; k < K; ++k) {
            const float e = (lapp[k] - la[k]) - ls2[k];
            le[perm[k]] = scaled ? s * e : e;
        }
    }
    free(ls1); free(lp1); free(ls2); free(lp2); free(la); free(lapp); free(le); free(alpha);
}
