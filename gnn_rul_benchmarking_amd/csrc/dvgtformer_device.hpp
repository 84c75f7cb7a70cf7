// DVGTformer: geometry, the flat / folded / partial-row / LDS layouts (stated once, for kernels and launcher) and the per-sample encoder
// forward and backward that csrc/dvgtformer.hip wraps in its two kernels.  One WORKGROUP owns one sample at a time.  Every phase is a
// loop "element e = tid, tid + nt, ..." over the phase's outputs with a barrier behind it and no cross-lane operation, so the same
// text runs as a plain serial function (tid 0 of 1, barrier = nothing) when DV_SERIAL is defined: that is how the arithmetic was
// checked against the fp64 oracle on a CPU.
//
// A half-block on tokens T and features F (temporal: T = L+1, F = N+1; spatial: T = N+1, F = L+1) reads the sample X [L+1][N+1] through
// (token stride, feature stride) = (N+1, 1) or (1, N+1): the transposes between the views are that index swap.  Fa = F + 1: the
// feature axis with the constant 1 that carries the biases into the folded operands M_h [Fa][Fa] and U_h [Fa][F] (dvgtformer.hip).
#pragma once
#include <stdint.h>

#ifdef DV_SERIAL
#include <cmath>
#define DV_FN inline
#define DV_HD inline
#define DV_SYNC() ((void)0)
#define DV_UNROLL
#else
// in front of a loop whose body reads a weight from global memory: eight loads in flight instead of one (the sums keep their order)
#define DV_UNROLL _Pragma("unroll 8")
#define DV_FN __device__ __forceinline__
#define DV_HD __host__ __device__ inline
#define DV_SYNC() __syncthreads()
#endif

namespace rulgnn {

constexpr int DV_MAX_BLOCKS = 8;        // RULGNN_DVGT_MAX_BLOCKS

struct DvGeom {
    int64_t B;
    int N, L, Np, Lp, E, H, nb, d[2], ff[2];
    float lam;
    int Tm, YN, TT, HN;                 // max(Lp, Np), max over the views of T Fa, Tm^2, max over the views of T d_ff
};

DV_HD int dv_max(int a, int b) { return a > b ? a : b; }

DV_HD void dv_derive(DvGeom* g) {
    g->Np = g->N + 1; g->Lp = g->L + 1; g->E = g->Np * g->Lp;
    g->Tm = dv_max(g->Lp, g->Np);
    g->YN = dv_max(g->Lp * (g->Np + 1), g->Np * (g->Lp + 1));
    g->TT = g->Tm * g->Tm;
    g->HN = dv_max(g->Lp * g->ff[0], g->Np * g->ff[1]);
}

DV_HD int dv_T(const DvGeom& g, int v) { return v ? g.Np : g.Lp; }
DV_HD int dv_F(const DvGeom& g, int v) { return v ? g.Lp : g.Np; }

// ---- flat parameter layout (the reference's named_parameters() order) --------------------------------------------------------------
// a half-block: H x (Wq [d][F], bq [d]) | H x (Wk, bk) | H x (Wv, bv) | W_O [F][H d], b_O [F] | LN1 g, b | LN2 g, b | W1 [ff][F], c1 [ff] |
// W2 [F][ff], c2 [F]; everything from b_O on ("direct") is copied into the partial rows as it is
struct DvHalfOff {
    int wsz, q, k, v, wo, bo, g1, b1, g2, b2, w1, c1, w2, c2, size, dirsz;
};
DV_HD DvHalfOff dv_half_off(int F, int d, int ff, int H) {
    DvHalfOff o;
    int t = 0;
    o.wsz = d * F + d;
    o.q = t; t += H * o.wsz;
    o.k = t; t += H * o.wsz;
    o.v = t; t += H * o.wsz;
    o.wo = t; t += F * H * d;
    o.bo = t; t += F;
    o.g1 = t; t += F;
    o.b1 = t; t += F;
    o.g2 = t; t += F;
    o.b2 = t; t += F;
    o.w1 = t; t += ff * F;
    o.c1 = t; t += ff;
    o.w2 = t; t += F * ff;
    o.c2 = t; t += F;
    o.size = t;
    o.dirsz = t - o.bo;
    return o;
}

// the whole buffer, the folded operands in the workspace (per (view, block): M [H][Fa][Fa] | U [H][Fa][F]; behind all of them the
// positional encoding [Lp][Np]) and a partial-gradient row (input stage as in the flat buffer | per (view, block): dM | dU | direct)
struct DvOff {
    int tv, xv, wt, bt, wx, bx, in, half[2], hsz[2], hw1, hb1, hw2, hb2, total;
    int fsz[2], fw_total, rsz[2], row_total;
};
DV_HD DvOff dv_offsets(const DvGeom& g) {
    DvOff o;
    int t = 0;
    o.tv = t; t += g.N;
    o.xv = t; t += g.Lp;
    o.wt = t; t += g.L * g.L;
    o.bt = t; t += g.L;
    o.wx = t; t += g.N * g.N;
    o.bx = t; t += g.N;
    o.in = t;
    for (int v = 0; v < 2; ++v) {
        const int F = dv_F(g, v);
        const DvHalfOff h = dv_half_off(F, g.d[v], g.ff[v], g.H);
        o.half[v] = t;
        o.hsz[v] = h.size;
        t += g.nb * h.size;
        o.fsz[v] = g.H * (F + 1) * (2 * F + 1);
        o.rsz[v] = o.fsz[v] + h.dirsz;
    }
    o.hw1 = t; t += 100 * g.E;
    o.hb1 = t; t += 100;
    o.hw2 = t; t += 100;
    o.hb2 = t; t += 1;
    o.total = t;
    o.fw_total = g.nb * (o.fsz[0] + o.fsz[1]);
    o.row_total = o.in + g.nb * (o.rsz[0] + o.rsz[1]);
    return o;
}
DV_HD int dv_fw_off(const DvGeom& g, const DvOff& o, int v, int blk) { return (v ? g.nb * o.fsz[0] : 0) + blk * o.fsz[v]; }
DV_HD int dv_row_off(const DvGeom& g, const DvOff& o, int v, int blk) { return o.in + (v ? g.nb * o.rsz[0] : 0) + blk * o.rsz[v]; }

// ---- LDS layout of a workgroup (floats) ----------------------------------------------------------------------------------------------
// X the half-block's input (the running sample), O the attention output then dO, D the FF's input, XU one head's X~ U_h and, behind the
// heads, the FF's output / its gradient, Y one head's X~ M_h, S a head's scores then softmax 1 (forward: then softmax 2), G the two
// graph softmaxes, H1 gelu(FF hidden), st six rows of per-token statistics.  Backward only: H2 the FF's pre-activation then its
// gradient; during the heads' backward H1 / H2 hold softmax 2 and d scores; dX the running gradient, dXU, dY, dG the gradients reaching
// the two graph softmaxes (summed over heads and blocks).  The input stage borrows Y (the raw window) and O (linear_t's output), the
// Pearson graphs XU (centred rows) and S (the correlation itself).
struct DvLds {
    int X, O, D, XU, Y, S, G[2], H1, st, H2, dX, dXU, dY, dG[2], total;
};
DV_HD DvLds dv_lds(const DvGeom& g, bool bwd) {
    DvLds l;
    int t = 0;
    const int hn = bwd ? dv_max(g.HN, g.TT) : g.HN;
    l.X = t; t += g.E;
    l.O = t; t += g.E;
    l.D = t; t += g.E;
    l.XU = t; t += g.E;
    l.Y = t; t += g.YN;
    l.S = t; t += g.TT;
    l.G[0] = t; t += g.Lp * g.Lp;
    l.G[1] = t; t += g.Np * g.Np;
    l.H1 = t; t += hn;
    l.st = t; t += 6 * g.Tm;
    l.H2 = l.dX = l.dXU = l.dY = l.dG[0] = l.dG[1] = t;
    if (bwd) {
        l.H2 = t; t += hn;
        l.dX = t; t += g.E;
        l.dXU = t; t += g.E;
        l.dY = t; t += g.YN;
        l.dG[0] = t; t += g.Lp * g.Lp;
        l.dG[1] = t; t += g.Np * g.Np;
    }
    l.total = t;
    return l;
}

// ---- fold / unfold, one element each ---------------------------------------------------------------------------------------------------
// W~[c][i]: the weight's column i < F or the bias at i == F
DV_FN float dv_wt(const float* w, int c, int i, int F, int d) { return i < F ? w[c * F + i] : w[d * F + c]; }

// element e of the folded operands (e < fw_total) or of the positional encoding behind them
DV_FN float dv_fold_elem(const DvGeom& g, const DvOff& o, const float* prm, int e) {
    if (e >= o.fw_total) {                                 // the positional encoding, as the reference rounds it (fp64 -> fp32)
        const int q = e - o.fw_total, pos = q / g.Np, col = q - pos * g.Np;
        const int i = col & ~1;
        if (i >= g.Np - 1) return 0.f;
        const double a = (double)pos / pow(10000.0, (double)(2 * i) / (double)g.Np);
        return (float)((col & 1) ? cos(a) : sin(a));
    }
    const int v = e >= g.nb * o.fsz[0];
    const int r0 = e - (v ? g.nb * o.fsz[0] : 0), blk = r0 / o.fsz[v], r = r0 - blk * o.fsz[v];
    const int F = dv_F(g, v), Fa = F + 1, d = g.d[v], H = g.H;
    const DvHalfOff ho = dv_half_off(F, d, g.ff[v], H);
    const float* hp = prm + o.half[v] + blk * ho.size;
    float a = 0.f;
    if (r < H * Fa * Fa) {
        const int h = r / (Fa * Fa), q = r - h * Fa * Fa, i = q / Fa, j = q - i * Fa;
        const float *wq = hp + ho.q + h * ho.wsz, *wk = hp + ho.k + h * ho.wsz;
        for (int c = 0; c < d; ++c) a = fmaf(dv_wt(wq, c, i, F, d), dv_wt(wk, c, j, F, d), a);
        a *= 1.0f / sqrtf((float)d);
    } else {
        const int r2 = r - H * Fa * Fa, h = r2 / (Fa * F), q = r2 - h * Fa * F, i = q / F, f = q - i * F;
        const float *wv = hp + ho.v + h * ho.wsz, *wo = hp + ho.wo + f * H * d + h * d;
        for (int c = 0; c < d; ++c) a = fmaf(dv_wt(wv, c, i, F, d), wo[c], a);
    }
    return a;
}

// flat gradient element e in front of the head (e < hw1) from the reduced partial row R
DV_FN float dv_unfold_elem(const DvGeom& g, const DvOff& o, const float* prm, const float* R, int e) {
    if (e < o.in) return R[e];
    const int v = e >= o.half[1];
    const int r0 = e - o.half[v], blk = r0 / o.hsz[v], r = r0 - blk * o.hsz[v];
    const int F = dv_F(g, v), Fa = F + 1, d = g.d[v], H = g.H;
    const DvHalfOff ho = dv_half_off(F, d, g.ff[v], H);
    const float* hp = prm + o.half[v] + blk * ho.size;
    const float* row = R + dv_row_off(g, o, v, blk);
    if (r >= ho.bo) return row[o.fsz[v] + r - ho.bo];
    float a = 0.f;
    if (r >= ho.wo) {                                      // dW_O[f][h d + c] = sum_i dU_h[i][f] W~v[c][i]
        const int q = r - ho.wo, f = q / (H * d), hc = q - f * H * d, h = hc / d, c = hc - h * d;
        const float* dU = row + H * Fa * Fa + h * Fa * F;
        const float* wv = hp + ho.v + h * ho.wsz;
        for (int i = 0; i < Fa; ++i) a = fmaf(dU[i * F + f], dv_wt(wv, c, i, F, d), a);
        return a;
    }
    const int which = r / (H * ho.wsz), r1 = r - which * H * ho.wsz, h = r1 / ho.wsz, q = r1 - h * ho.wsz;
    const int c = q < d * F ? q / F : q - d * F, i = q < d * F ? q - c * F : F;
    const float* dM = row + h * Fa * Fa;
    const float sc = 1.0f / sqrtf((float)d);
    if (which == 0) {                                      // dW~q[c][i] = sum_j dM[i][j] W~k[c][j] / sqrt(d)
        const float* wk = hp + ho.k + h * ho.wsz;
        for (int j = 0; j < Fa; ++j) a = fmaf(dM[i * Fa + j], dv_wt(wk, c, j, F, d), a);
        a *= sc;
    } else if (which == 1) {                               // dW~k[c][i] = sum_j dM[j][i] W~q[c][j] / sqrt(d); the bias: exactly 0
        if (i < F) {
            const float* wq = hp + ho.q + h * ho.wsz;
            for (int j = 0; j < Fa; ++j) a = fmaf(dM[j * Fa + i], dv_wt(wq, c, j, F, d), a);
            a *= sc;
        }
    } else {                                               // dW~v[c][i] = sum_f dU[i][f] W_O[f][h d + c]
        const float* dU = row + H * Fa * Fa + h * Fa * F;
        for (int f = 0; f < F; ++f) a = fmaf(dU[i * F + f], hp[ho.wo + f * H * d + h * d + c], a);
    }
    return a;
}

struct DvDrop {
    uint32_t key[DV_MAX_BLOCKS], thr, sample_offset;
    float scale;
};

#ifdef DV_SERIAL
inline uint32_t dv_hash(uint32_t h) {
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}
#else
DV_FN uint32_t dv_hash(uint32_t h) { return lowbias32(h); }
#endif

DV_FN float dv_keep(const DvDrop& d, int blk, uint32_t ctr) {
    if (d.thr == 0u) return 1.f;
    return dv_hash(ctr ^ d.key[blk]) >= d.thr ? d.scale : 0.f;
}

DV_FN float dv_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
DV_FN float dv_gelu_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * expf(-0.5f * x * x) * 0.39894228040143268f;
}

struct DvCtx {
    int tid, nt;
    float* lds;
};

// what a half-block call knows
struct DvHalf {
    int v, blk, T, F, Fa, st, sf, d, ff;
    DvHalfOff ho;
    const float* hp;        // the half-block's parameters
    const float *Mw, *Uw;   // folded operands
};
DV_FN DvHalf dv_half(const DvGeom& g, const DvOff& o, int v, int blk, const float* prm, const float* fw) {
    DvHalf h;
    h.v = v; h.blk = blk; h.T = dv_T(g, v); h.F = dv_F(g, v); h.Fa = h.F + 1;
    h.st = v ? 1 : g.Np; h.sf = v ? g.Np : 1;
    h.d = g.d[v]; h.ff = g.ff[v];
    h.ho = dv_half_off(h.F, h.d, h.ff, g.H);
    h.hp = prm + o.half[v] + blk * h.ho.size;
    h.Mw = fw + dv_fw_off(g, o, v, blk);
    h.Uw = h.Mw + g.H * h.Fa * h.Fa;
    return h;
}
// canonical element e of [Lp][Np] -> (token, feature) of the view
DV_FN void dv_tf(const DvGeom& g, int v, int e, int& t, int& f) {
    const int l = e / g.Np, n = e - l * g.Np;
    t = v ? n : l;
    f = v ? l : n;
}

#define DV_AT(buf, t, f) (buf)[(t) * hb.st + (f) * hb.sf]

// Pearson correlation of the T rows of the view: centred rows -> cbuf (canonical layout), norms -> nrm [T], A [T][T].  A constant row
// gives 0 / 0 = NaN, as the reference; no epsilon.
DV_FN void dv_pcc(const DvCtx& c, const DvGeom& g, int v, const float* Xc, float* cbuf, float* nrm, float* A) {
    const int T = dv_T(g, v), F = dv_F(g, v), st = v ? 1 : g.Np, sf = v ? g.Np : 1;
    for (int t = c.tid; t < T; t += c.nt) {
        float m = 0.f;
        for (int f = 0; f < F; ++f) m += Xc[t * st + f * sf];
        m /= (float)F;
        float ss = 0.f;
        for (int f = 0; f < F; ++f) {
            const float x = Xc[t * st + f * sf] - m;
            cbuf[t * st + f * sf] = x;
            ss = fmaf(x, x, ss);
        }
        nrm[t] = sqrtf(ss);
    }
    DV_SYNC();
    for (int e = c.tid; e < T * T; e += c.nt) {
        const int t = e / T, u = e - t * T;
        float a = 0.f;
        for (int f = 0; f < F; ++f) a = fmaf(cbuf[t * st + f * sf], cbuf[u * st + f * sf], a);
        A[e] = a / (nrm[t] * nrm[u]);
    }
    DV_SYNC();
}

// G = softmax_row(relu(A)); relu keeps a NaN
DV_FN void dv_graph_softmax(const DvCtx& c, int T, const float* A, float* G) {
    for (int t = c.tid; t < T; t += c.nt) {
        float m = 0.f;
        for (int u = 0; u < T; ++u) {
            const float a = A[t * T + u];
            m = fmaxf(m, a < 0.f ? 0.f : a);
        }
        float s = 0.f;
        for (int u = 0; u < T; ++u) {
            const float a = A[t * T + u];
            const float e = expf((a < 0.f ? 0.f : a) - m);
            G[t * T + u] = e;
            s += e;
        }
        const float inv = 1.f / s;
        for (int u = 0; u < T; ++u) G[t * T + u] *= inv;
    }
    DV_SYNC();
}

// one head: Y = X~ M_h, XU = X~ U_h, S = softmax(Y X~^T), Pout = softmax((1 - lam) S + lam G) (Pout may be S); barrier behind
DV_FN void dv_head_scores(const DvCtx& c, const DvGeom& g, const DvHalf& hb, int h, const float* X, const float* G, float* Y, float* XU, float* S,
                          float* Pout) {
    const int T = hb.T, F = hb.F, Fa = hb.Fa;
    const float* M = hb.Mw + h * Fa * Fa;
    const float* U = hb.Uw + h * Fa * F;
    for (int e = c.tid; e < T * Fa; e += c.nt) {
        const int t = e / Fa, j = e - t * Fa;
        float a = M[F * Fa + j];
        DV_UNROLL
        for (int i = 0; i < F; ++i) a = fmaf(DV_AT(X, t, i), M[i * Fa + j], a);
        Y[e] = a;
    }
    for (int e = c.tid; e < T * F; e += c.nt) {
        const int t = e / F, f = e - t * F;
        float a = U[F * F + f];
        DV_UNROLL
        for (int i = 0; i < F; ++i) a = fmaf(DV_AT(X, t, i), U[i * F + f], a);
        XU[e] = a;
    }
    DV_SYNC();
    for (int e = c.tid; e < T * T; e += c.nt) {
        const int t = e / T, u = e - t * T;
        float a = Y[t * Fa + F];
        for (int j = 0; j < F; ++j) a = fmaf(Y[t * Fa + j], DV_AT(X, u, j), a);
        S[e] = a;
    }
    DV_SYNC();
    const float lam = g.lam, oml = 1.f - g.lam;
    for (int t = c.tid; t < T; t += c.nt) {
        float* s = S + t * T;
        float* p = Pout + t * T;
        const float* gr = G + t * T;
        float m = s[0];
        for (int u = 1; u < T; ++u) m = fmaxf(m, s[u]);
        float sum = 0.f;
        for (int u = 0; u < T; ++u) {
            const float e = expf(s[u] - m);
            s[u] = e;
            sum += e;
        }
        float inv = 1.f / sum, m2 = -INFINITY;
        for (int u = 0; u < T; ++u) {
            const float p1 = s[u] * inv;
            s[u] = p1;
            m2 = fmaxf(m2, oml * p1 + lam * gr[u]);
        }
        sum = 0.f;
        for (int u = 0; u < T; ++u) {
            const float e = expf(oml * s[u] + lam * gr[u] - m2);
            sum += e;
        }
        inv = 1.f / sum;
        // (p may be s: softmax 1 is read before softmax 2 overwrites it)
        for (int u = 0; u < T; ++u) p[u] = expf(oml * s[u] + lam * gr[u] - m2) * inv;
    }
    DV_SYNC();
}

// LayerNorm statistics of the rows of the view: mu[t], rs[t] = 1 / sqrt(var + 1e-5)
DV_FN void dv_ln_stats(const DvCtx& c, const DvHalf& hb, const float* Z, float* mu, float* rs) {
    for (int t = c.tid; t < hb.T; t += c.nt) {
        float m = 0.f;
        for (int f = 0; f < hb.F; ++f) m += DV_AT(Z, t, f);
        m /= (float)hb.F;
        float var = 0.f;
        for (int f = 0; f < hb.F; ++f) {
            const float x = DV_AT(Z, t, f) - m;
            var = fmaf(x, x, var);
        }
        mu[t] = m;
        rs[t] = 1.f / sqrtf(var / (float)hb.F + 1e-5f);
    }
    DV_SYNC();
}

// Forward of one half-block on the sample in l.X.  Leaves O (attention output before LN1), D, H1 = gelu(hidden) (with `bwd` also H2 =
// the pre-activation), XU = the FF's output, st = {mu1, rs1, mu2, rs2}; without `bwd` the half-block's output replaces X.
DV_FN void dv_half_fwd(const DvCtx& c, const DvGeom& g, const DvLds& l, const DvHalf& hb, const DvDrop& drop, int64_t sample, bool bwd) {
    float *X = c.lds + l.X, *O = c.lds + l.O, *D = c.lds + l.D, *XU = c.lds + l.XU, *Y = c.lds + l.Y, *S = c.lds + l.S;
    float *H1 = c.lds + l.H1, *H2 = c.lds + l.H2, *st = c.lds + l.st;
    const float* G = c.lds + l.G[hb.v];
    const int T = hb.T, F = hb.F, ff = hb.ff;
    const float* hp = hb.hp;
    for (int e = c.tid; e < g.E; e += c.nt) {
        int t, f;
        dv_tf(g, hb.v, e, t, f);
        O[e] = hp[hb.ho.bo + f];
    }
    // (the first barrier inside dv_head_scores orders this against the first accumulation)
    for (int h = 0; h < g.H; ++h) {
        dv_head_scores(c, g, hb, h, X, G, Y, XU, S, S);
        for (int e = c.tid; e < g.E; e += c.nt) {
            int t, f;
            dv_tf(g, hb.v, e, t, f);
            float a = O[e];
            for (int u = 0; u < T; ++u) a = fmaf(S[t * T + u], XU[u * F + f], a);
            O[e] = a;
        }
        DV_SYNC();
    }
    dv_ln_stats(c, hb, O, st, st + g.Tm);
    const uint32_t ctr0 = ((uint32_t)sample + drop.sample_offset) * (uint32_t)g.E;
    for (int e = c.tid; e < g.E; e += c.nt) {
        int t, f;
        dv_tf(g, hb.v, e, t, f);
        const float r = (O[e] - st[t]) * st[g.Tm + t] * hp[hb.ho.g1 + f] + hp[hb.ho.b1 + f] + X[e];
        D[e] = hb.v == 0 ? r * dv_keep(drop, hb.blk, ctr0 + (uint32_t)e) : r;
    }
    DV_SYNC();
    for (int e = c.tid; e < T * ff; e += c.nt) {
        const int t = e / ff, j = e - t * ff;
        float a = hp[hb.ho.c1 + j];
        DV_UNROLL
        for (int f = 0; f < F; ++f) a = fmaf(DV_AT(D, t, f), hp[hb.ho.w1 + j * F + f], a);
        if (bwd) H2[e] = a;
        H1[e] = dv_gelu(a);
    }
    DV_SYNC();
    for (int e = c.tid; e < g.E; e += c.nt) {
        int t, f;
        dv_tf(g, hb.v, e, t, f);
        float a = hp[hb.ho.c2 + f];
        DV_UNROLL
        for (int j = 0; j < ff; ++j) a = fmaf(H1[t * ff + j], hp[hb.ho.w2 + f * ff + j], a);
        XU[e] = a;
    }
    DV_SYNC();
    dv_ln_stats(c, hb, XU, st + 2 * g.Tm, st + 3 * g.Tm);
    if (!bwd) {
        for (int e = c.tid; e < g.E; e += c.nt) {
            int t, f;
            dv_tf(g, hb.v, e, t, f);
            X[e] = (XU[e] - st[2 * g.Tm + t]) * st[3 * g.Tm + t] * hp[hb.ho.g2 + f] + hp[hb.ho.b2 + f] + D[e];
        }
        DV_SYNC();
    }
}

// Input stage and graphs of one sample: x [N][L] -> X (with the positional encoding) in l.X, both graph softmaxes in l.G.
DV_FN void dv_input_fwd(const DvCtx& c, const DvGeom& g, const DvOff& o, const DvLds& l, const float* x, const float* prm, const float* pe) {
    float *X = c.lds + l.X, *XI = c.lds + l.Y, *X1 = c.lds + l.O;
    const int N = g.N, L = g.L, Np = g.Np;
    for (int e = c.tid; e < N * L; e += c.nt) XI[e] = x[e];
    DV_SYNC();
    for (int e = c.tid; e < N * L; e += c.nt) {
        const int n = e / L, k = e - n * L;
        float a = prm[o.bt + k];
        DV_UNROLL
        for (int q = 0; q < L; ++q) a = fmaf(XI[n * L + q], prm[o.wt + k * L + q], a);
        X1[e] = a;
    }
    DV_SYNC();
    for (int e = c.tid; e < g.E; e += c.nt) {
        const int q = e / Np, m = e - q * Np;
        float a;
        if (m == N) a = prm[o.xv + q];
        else if (q == L) a = prm[o.tv + m];
        else {
            a = prm[o.bx + m];
            DV_UNROLL
            for (int n = 0; n < N; ++n) a = fmaf(X1[n * L + q], prm[o.wx + m * N + n], a);
        }
        X[e] = a;
    }
    DV_SYNC();
    for (int v = 0; v < 2; ++v) {
        dv_pcc(c, g, v, X, c.lds + l.XU, c.lds + l.st + 4 * g.Tm, c.lds + l.S);
        dv_graph_softmax(c, dv_T(g, v), c.lds + l.S, c.lds + l.G[v]);
    }
    for (int e = c.tid; e < g.E; e += c.nt) X[e] += pe[e];
    DV_SYNC();
}

// Encoder forward of one sample; hin: the sample's slot-0 record ([slot][B][E], `slot_stride` floats apart): the inputs of the 2 nb
// half-blocks (slot 0 = X behind the input stage and the positional encoding) and, last, the encoder output.
DV_FN void dv_sample_fwd(const DvCtx& c, const DvGeom& g, const DvOff& o, const DvLds& l, const DvDrop& drop, int64_t sample, const float* x,
                         const float* prm, const float* fw, float* hin, int64_t slot_stride) {
    dv_input_fwd(c, g, o, l, x, prm, fw + o.fw_total);
    float* X = c.lds + l.X;
    for (int s = 0; s < 2 * g.nb; ++s) {
        for (int e = c.tid; e < g.E; e += c.nt) hin[s * slot_stride + e] = X[e];
        const DvHalf hb = dv_half(g, o, s & 1, s >> 1, prm, fw);
        dv_half_fwd(c, g, l, hb, drop, sample, false);
    }
    for (int e = c.tid; e < g.E; e += c.nt) hin[2 * g.nb * slot_stride + e] = X[e];
    DV_SYNC();
}

// part[idx] += val: the workgroup's partial-gradient row; an index has one owner thread per phase, the same for every sample, and the
// workgroup's first sample starts the sum.  The old value is loaded in front of the loop that computes `val`, so that its latency
// hides behind the loop.
#define DV_ACC_LOAD(name, idx)          \
    float* name##_p = part + (idx);     \
    const float name##_old = first ? 0.f : *name##_p
#define DV_ACC_STORE(name, val) *name##_p = name##_old + (val)
#define DV_ACC(idx, val)                \
    do {                                \
        DV_ACC_LOAD(acc, idx);          \
        DV_ACC_STORE(acc, val);         \
    } while (0)

// LayerNorm backward on the view: dy in `dYb` (kept), the normalised input from (Z, mu, rs); parameter gradients to the row, dz replaces Z
DV_FN void dv_ln_bwd(const DvCtx& c, const DvHalf& hb, const float* dYb, float* Z, const float* mu, const float* rs, const float* gam,
                     float* part, int ig, int ib, bool first) {
    const int T = hb.T, F = hb.F;
    for (int f = c.tid; f < F; f += c.nt) {
        DV_ACC_LOAD(ga, ig + f);
        DV_ACC_LOAD(gb, ib + f);
        float a = 0.f, b = 0.f;
        for (int t = 0; t < T; ++t) {
            const float dy = DV_AT(dYb, t, f);
            a = fmaf(dy, (DV_AT(Z, t, f) - mu[t]) * rs[t], a);
            b += dy;
        }
        DV_ACC_STORE(ga, a);
        DV_ACC_STORE(gb, b);
    }
    DV_SYNC();
    for (int t = c.tid; t < T; t += c.nt) {
        float m1 = 0.f, m2 = 0.f;
        for (int f = 0; f < F; ++f) {
            const float dxh = DV_AT(dYb, t, f) * gam[f], xh = (DV_AT(Z, t, f) - mu[t]) * rs[t];
            m1 += dxh;
            m2 = fmaf(dxh, xh, m2);
        }
        m1 /= (float)F;
        m2 /= (float)F;
        for (int f = 0; f < F; ++f) {
            const float dxh = DV_AT(dYb, t, f) * gam[f], xh = (DV_AT(Z, t, f) - mu[t]) * rs[t];
            DV_AT(Z, t, f) = (dxh - m1 - xh * m2) * rs[t];
        }
    }
    DV_SYNC();
}

// Backward of one half-block: its input in l.X, d output in l.dX; leaves d input in l.dX, adds to dG of the view and to the row.
DV_FN void dv_half_bwd(const DvCtx& c, const DvGeom& g, const DvOff& o, const DvLds& l, const DvHalf& hb, const DvDrop& drop, int64_t sample,
                       float* part_row, bool first) {
    dv_half_fwd(c, g, l, hb, drop, sample, true);
    float *X = c.lds + l.X, *O = c.lds + l.O, *D = c.lds + l.D, *XU = c.lds + l.XU, *Y = c.lds + l.Y, *S = c.lds + l.S;
    float *H1 = c.lds + l.H1, *H2 = c.lds + l.H2, *st = c.lds + l.st, *dX = c.lds + l.dX, *dXU = c.lds + l.dXU, *dY = c.lds + l.dY;
    float* dG = c.lds + l.dG[hb.v];
    const float* G = c.lds + l.G[hb.v];
    const int T = hb.T, F = hb.F, Fa = hb.Fa, ff = hb.ff, Tm = g.Tm;
    const float* hp = hb.hp;
    const DvHalfOff& ho = hb.ho;
    float* part = part_row + dv_row_off(g, o, hb.v, hb.blk);
    const int dir = o.fsz[hb.v] - ho.bo;               // row index of flat within-half offset q >= bo: dir + q
    const int iM = 0, iU = g.H * Fa * Fa;
    // LN2 and the FF
    float* FFo = XU;
    dv_ln_bwd(c, hb, dX, FFo, st + 2 * Tm, st + 3 * Tm, hp + ho.g2, part, dir + ho.g2, dir + ho.b2, first);
    for (int e = c.tid; e < F * ff; e += c.nt) {
        const int f = e / ff, j = e - f * ff;
        DV_ACC_LOAD(acc, dir + ho.w2 + e);
        float a = 0.f;
        for (int t = 0; t < T; ++t) a = fmaf(DV_AT(FFo, t, f), H1[t * ff + j], a);
        DV_ACC_STORE(acc, a);
    }
    for (int f = c.tid; f < F; f += c.nt) {
        DV_ACC_LOAD(acc, dir + ho.c2 + f);
        float a = 0.f;
        for (int t = 0; t < T; ++t) a += DV_AT(FFo, t, f);
        DV_ACC_STORE(acc, a);
    }
    for (int e = c.tid; e < T * ff; e += c.nt) {
        const int t = e / ff, j = e - t * ff;
        float a = 0.f;
        DV_UNROLL
        for (int f = 0; f < F; ++f) a = fmaf(DV_AT(FFo, t, f), hp[ho.w2 + f * ff + j], a);
        H2[e] = a * dv_gelu_grad(H2[e]);
    }
    DV_SYNC();
    for (int e = c.tid; e < ff * F; e += c.nt) {
        const int j = e / F, f = e - j * F;
        DV_ACC_LOAD(acc, dir + ho.w1 + e);
        float a = 0.f;
        for (int t = 0; t < T; ++t) a = fmaf(H2[t * ff + j], DV_AT(D, t, f), a);
        DV_ACC_STORE(acc, a);
    }
    for (int j = c.tid; j < ff; j += c.nt) {
        DV_ACC_LOAD(acc, dir + ho.c1 + j);
        float a = 0.f;
        for (int t = 0; t < T; ++t) a += H2[t * ff + j];
        DV_ACC_STORE(acc, a);
    }
    const uint32_t ctr0 = ((uint32_t)sample + drop.sample_offset) * (uint32_t)g.E;
    for (int e = c.tid; e < g.E; e += c.nt) {
        int t, f;
        dv_tf(g, hb.v, e, t, f);
        float a = dX[e];
        DV_UNROLL
        for (int j = 0; j < ff; ++j) a = fmaf(H2[t * ff + j], hp[ho.w1 + j * F + f], a);
        dX[e] = hb.v == 0 ? a * dv_keep(drop, hb.blk, ctr0 + (uint32_t)e) : a;
    }
    DV_SYNC();
    // LN1: dX now holds d R, which is also the residual's share of d input; O becomes d O
    dv_ln_bwd(c, hb, dX, O, st, st + Tm, hp + ho.g1, part, dir + ho.g1, dir + ho.b1, first);
    for (int f = c.tid; f < F; f += c.nt) {
        DV_ACC_LOAD(acc, dir + ho.bo + f);
        float a = 0.f;
        for (int t = 0; t < T; ++t) a += DV_AT(O, t, f);
        DV_ACC_STORE(acc, a);
    }
    float *PB = H1, *Cb = H2;
    const float lam = g.lam, oml = 1.f - g.lam;
    for (int h = 0; h < g.H; ++h) {
        const float* M = hb.Mw + h * Fa * Fa;
        const float* U = hb.Uw + h * Fa * F;
        dv_head_scores(c, g, hb, h, X, G, Y, XU, S, PB);
        for (int e = c.tid; e < T * F; e += c.nt) {
            const int u = e / F, f = e - u * F;
            float a = 0.f;
            for (int t = 0; t < T; ++t) a = fmaf(PB[t * T + u], DV_AT(O, t, f), a);
            dXU[e] = a;
        }
        for (int e = c.tid; e < T * T; e += c.nt) {
            const int t = e / T, u = e - t * T;
            float a = 0.f;
            for (int f = 0; f < F; ++f) a = fmaf(DV_AT(O, t, f), XU[u * F + f], a);
            Cb[e] = a;
        }
        DV_SYNC();
        for (int t = c.tid; t < T; t += c.nt) {
            float r = 0.f;
            for (int u = 0; u < T; ++u) r = fmaf(Cb[t * T + u], PB[t * T + u], r);
            float r1 = 0.f;
            for (int u = 0; u < T; ++u) {
                const float dz = PB[t * T + u] * (Cb[t * T + u] - r);
                dG[t * T + u] = fmaf(lam, dz, dG[t * T + u]);
                const float dp1 = oml * dz;
                Cb[t * T + u] = dp1;
                r1 = fmaf(dp1, S[t * T + u], r1);
            }
            for (int u = 0; u < T; ++u) Cb[t * T + u] = S[t * T + u] * (Cb[t * T + u] - r1);
        }
        DV_SYNC();
        for (int e = c.tid; e < T * Fa; e += c.nt) {
            const int t = e / Fa, j = e - t * Fa;
            float a = 0.f;
            if (j < F) for (int u = 0; u < T; ++u) a = fmaf(Cb[t * T + u], DV_AT(X, u, j), a);
            else for (int u = 0; u < T; ++u) a += Cb[t * T + u];
            dY[e] = a;
        }
        for (int e = c.tid; e < Fa * F; e += c.nt) {
            const int i = e / F, f = e - i * F;
            DV_ACC_LOAD(acc, iU + h * Fa * F + e);
            float a = 0.f;
            if (i < F) for (int t = 0; t < T; ++t) a = fmaf(DV_AT(X, t, i), dXU[t * F + f], a);
            else for (int t = 0; t < T; ++t) a += dXU[t * F + f];
            DV_ACC_STORE(acc, a);
        }
        DV_SYNC();
        for (int e = c.tid; e < Fa * Fa; e += c.nt) {
            const int i = e / Fa, j = e - i * Fa;
            DV_ACC_LOAD(acc, iM + h * Fa * Fa + e);
            float a = 0.f;
            if (i < F) for (int t = 0; t < T; ++t) a = fmaf(DV_AT(X, t, i), dY[t * Fa + j], a);
            else for (int t = 0; t < T; ++t) a += dY[t * Fa + j];
            DV_ACC_STORE(acc, a);
        }
        for (int e = c.tid; e < g.E; e += c.nt) {
            int t, i;
            dv_tf(g, hb.v, e, t, i);
            float a = dX[e];
            for (int u = 0; u < T; ++u) a = fmaf(Cb[u * T + t], Y[u * Fa + i], a);
            DV_UNROLL
            for (int f = 0; f < F; ++f) a = fmaf(dXU[t * F + f], U[i * F + f], a);
            DV_UNROLL
            for (int j = 0; j < Fa; ++j) a = fmaf(dY[t * Fa + j], M[i * Fa + j], a);
            dX[e] = a;
        }
        DV_SYNC();
    }
}

// Gradient through the two Pearson graphs: l.X holds X WITHOUT the positional encoding, l.dG the gradients reaching the graph
// softmaxes; adds to l.dX.
DV_FN void dv_graph_bwd(const DvCtx& c, const DvGeom& g, const DvLds& l) {
    float *X = c.lds + l.X, *cb = c.lds + l.XU, *A = c.lds + l.S, *dc = c.lds + l.D, *dX = c.lds + l.dX;
    float *nrm = c.lds + l.st + 4 * g.Tm, *dn = c.lds + l.st + 5 * g.Tm, *mean = c.lds + l.st;
    for (int v = 0; v < 2; ++v) {
        const int T = dv_T(g, v), F = dv_F(g, v), st = v ? 1 : g.Np, sf = v ? g.Np : 1;
        const float* G = c.lds + l.G[v];
        float* dA = c.lds + l.dG[v];
        dv_pcc(c, g, v, X, cb, nrm, A);
        for (int t = c.tid; t < T; t += c.nt) {
            float r = 0.f;
            for (int u = 0; u < T; ++u) r = fmaf(dA[t * T + u], G[t * T + u], r);
            for (int u = 0; u < T; ++u) dA[t * T + u] = A[t * T + u] > 0.f ? G[t * T + u] * (dA[t * T + u] - r) : 0.f;
        }
        DV_SYNC();
        for (int t = c.tid; t < T; t += c.nt) {
            float w = 0.f;
            for (int u = 0; u < T; ++u) w += dA[t * T + u] * A[t * T + u] + dA[u * T + t] * A[u * T + t];
            dn[t] = -w / nrm[t];
        }
        DV_SYNC();
        for (int e = c.tid; e < g.E; e += c.nt) {
            int t, f;
            dv_tf(g, v, e, t, f);
            float a = 0.f;
            for (int u = 0; u < T; ++u) a = fmaf((dA[t * T + u] + dA[u * T + t]) / (nrm[t] * nrm[u]), cb[u * st + f * sf], a);
            dc[e] = a + dn[t] * cb[e] / nrm[t];
        }
        DV_SYNC();
        for (int t = c.tid; t < T; t += c.nt) {
            float m = 0.f;
            for (int f = 0; f < F; ++f) m += dc[t * st + f * sf];
            mean[t] = m / (float)F;
        }
        DV_SYNC();
        for (int e = c.tid; e < g.E; e += c.nt) {
            int t, f;
            dv_tf(g, v, e, t, f);
            dX[e] += dc[e] - mean[t];
        }
        DV_SYNC();
    }
}

// Encoder backward of one sample: d enc [E] -> the workgroup's partial row (every folded / direct / input-stage gradient).
DV_FN void dv_sample_bwd(const DvCtx& c, const DvGeom& g, const DvOff& o, const DvLds& l, const DvDrop& drop, int64_t sample, const float* x,
                         const float* prm, const float* fw, const float* hin, int64_t slot_stride, const float* denc, float* part, bool first) {
    float *X = c.lds + l.X, *dX = c.lds + l.dX;
    const float* pe = fw + o.fw_total;
    const int N = g.N, L = g.L, Np = g.Np;
    // the graph softmaxes from X without the positional encoding (slot 0 holds X with it)
    for (int e = c.tid; e < g.E; e += c.nt) {
        X[e] = hin[e] - pe[e];
        dX[e] = denc[e];
    }
    for (int e = c.tid; e < g.Lp * g.Lp; e += c.nt) c.lds[l.dG[0] + e] = 0.f;
    for (int e = c.tid; e < g.Np * g.Np; e += c.nt) c.lds[l.dG[1] + e] = 0.f;
    DV_SYNC();
    for (int v = 0; v < 2; ++v) {
        dv_pcc(c, g, v, X, c.lds + l.XU, c.lds + l.st + 4 * g.Tm, c.lds + l.S);
        dv_graph_softmax(c, dv_T(g, v), c.lds + l.S, c.lds + l.G[v]);
    }
    for (int s = 2 * g.nb - 1; s >= 0; --s) {
        for (int e = c.tid; e < g.E; e += c.nt) X[e] = hin[s * slot_stride + e];
        DV_SYNC();
        const DvHalf hb = dv_half(g, o, s & 1, s >> 1, prm, fw);
        dv_half_bwd(c, g, o, l, hb, drop, sample, part, first);
    }
    for (int e = c.tid; e < g.E; e += c.nt) X[e] = hin[e] - pe[e];
    DV_SYNC();
    dv_graph_bwd(c, g, l);
    // input stage: dX is d X [Lp][Np]
    float *XI = c.lds + l.Y, *X1 = c.lds + l.O, *dX1 = c.lds + l.dXU;
    for (int e = c.tid; e < N * L; e += c.nt) XI[e] = x[e];
    for (int m = c.tid; m < N; m += c.nt) DV_ACC(o.tv + m, dX[L * Np + m]);
    for (int q = c.tid; q < g.Lp; q += c.nt) DV_ACC(o.xv + q, dX[q * Np + N]);
    DV_SYNC();
    for (int e = c.tid; e < N * L; e += c.nt) {
        const int n = e / L, k = e - n * L;
        float a = prm[o.bt + k];
        DV_UNROLL
        for (int q = 0; q < L; ++q) a = fmaf(XI[n * L + q], prm[o.wt + k * L + q], a);
        X1[e] = a;
    }
    DV_SYNC();
    for (int e = c.tid; e < N * N; e += c.nt) {
        const int m = e / N, n = e - m * N;
        DV_ACC_LOAD(acc, o.wx + e);
        float a = 0.f;
        for (int q = 0; q < L; ++q) a = fmaf(dX[q * Np + m], X1[n * L + q], a);
        DV_ACC_STORE(acc, a);
    }
    for (int m = c.tid; m < N; m += c.nt) {
        DV_ACC_LOAD(acc, o.bx + m);
        float a = 0.f;
        for (int q = 0; q < L; ++q) a += dX[q * Np + m];
        DV_ACC_STORE(acc, a);
    }
    for (int e = c.tid; e < N * L; e += c.nt) {
        const int n = e / L, q = e - n * L;
        float a = 0.f;
        DV_UNROLL
        for (int m = 0; m < N; ++m) a = fmaf(dX[q * Np + m], prm[o.wx + m * N + n], a);
        dX1[e] = a;
    }
    DV_SYNC();
    for (int e = c.tid; e < L * L; e += c.nt) {
        const int k = e / L, q = e - k * L;
        DV_ACC_LOAD(acc, o.wt + e);
        float a = 0.f;
        for (int n = 0; n < N; ++n) a = fmaf(dX1[n * L + k], XI[n * L + q], a);
        DV_ACC_STORE(acc, a);
    }
    for (int k = c.tid; k < L; k += c.nt) {
        DV_ACC_LOAD(acc, o.bt + k);
        float a = 0.f;
        for (int n = 0; n < N; ++n) a += dX1[n * L + k];
        DV_ACC_STORE(acc, a);
    }
    DV_SYNC();
}

}  // namespace rulgnn
