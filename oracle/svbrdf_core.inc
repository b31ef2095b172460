/*
 * svbrdf_core.inc -- TEST INFRASTRUCTURE (oracle), not product code.
 *
 * Per-pixel restatement of the reference's Cook-Torrance/GGX point-light
 * shading and of the rendering loss, parameterised on the arithmetic type:
 *
 *     #define REAL   float | double
 *     #define FN(x)  x##_f32 | x##_f64
 *
 * The float instantiation follows the reference's fp32 operation ORDER
 * (one rounding per torch op, dot products summed (p0+p1)+p2, true divisions,
 * correctly rounded sqrt, no FMA contraction -- compile with
 * -ffp-contract=off) so that it reproduces the reference's renderings to the
 * last few ULP.  The double instantiation evaluates the same formulas on the
 * same fp32-valued inputs and is used to show the float path is not LESS
 * accurate than the reference.
 *
 * Reference lines restated (development/multiImage_pytorch/):
 *   renderers.py:8-12    dot_product, normalize
 *   renderers.py:15-16   xi (Heaviside; ==1 on this path, zero gradient)
 *   renderers.py:18-20   compute_diffuse_term
 *   renderers.py:22-27   compute_microfacet_distribution (GGX D)
 *   renderers.py:29-32   compute_fresnel (Schlick, real pow(.,5))
 *   renderers.py:34-41   compute_g1 / compute_geometry (Smith)
 *   renderers.py:43-60   compute_specular_term
 *   renderers.py:62-65   evaluate_brdf
 *   renderers.py:67-104  LocalRenderer.render
 *   losses.py:29-52      RenderingLoss.forward (log(x+0.1), L1 mean)
 * The backward is the analytic adjoint of exactly that computation with
 * PyTorch's sub-gradient conventions (clamp(min=m) passes gradient iff
 * x >= m, sign(0) = 0), cf. SURVEY.md section 8a.
 */

#ifndef REAL
#error "define REAL and FN before including svbrdf_core.inc"
#endif

/* torch multiplies/divides an fp32 tensor by the python float math.pi after
 * casting it to fp32 (probe: x/math.pi == x / float32(pi) bit for bit). */
#define PI_R ((REAL)3.14159274101257324219f)

typedef struct {
    REAL wo[3], wi[3], h[3];
    REAL fall;   /* 1 / (sqrt(|L|^2))^2          renderers.py:99  */
    REAL p;      /* (1 - VH)^5                    renderers.py:32  */
} FN(geom_t);

typedef struct {
    /* raw (pre-clamp) dot products, needed for the clamp masks */
    REAL nh_raw, vn_raw, ln_raw;
    REAL NH, VN, LN, LNp;
    REAL r[3], A[3], F[3], G1V[3], G1L[3], wV[3], wL[3], D[3];
    REAL den[3], den_raw[3];
    REAL spec[3], f[3], E[3];
    REAL uV, uL;            /* (1-XN^2)/XN^2 evaluated for the backward */
} FN(ctx_t);

static inline REAL FN(dot3)(const REAL *a, const REAL *b)
{
    /* torch.sum(a*b, dim=-3): products rounded one by one, (p0+p1)+p2 */
    REAL p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
    return (p0 + p1) + p2;
}

static inline REAL FN(maxr)(REAL a, REAL b) { return a > b ? a : b; }

/* map-independent part: renderers.py:73-82, 91-93, 45, 49, 32, 99 */
static inline void FN(geometry)(const float *sc, REAL x, REAL y, FN(geom_t) *g)
{
    REAL rc[3] = { (REAL)sc[0] - x, (REAL)sc[1] - y, (REAL)sc[2] - (REAL)0 };
    REAL rl[3] = { (REAL)sc[3] - x, (REAL)sc[4] - y, (REAL)sc[5] - (REAL)0 };
    REAL lc = SQRT_R(FN(dot3)(rc, rc));
    REAL d2 = FN(dot3)(rl, rl);
    REAL ll = SQRT_R(d2);
    REAL hs[3];
    int k;
    for (k = 0; k < 3; ++k) {
        g->wo[k] = rc[k] / lc;
        g->wi[k] = rl[k] / ll;
    }
    for (k = 0; k < 3; ++k)
        hs[k] = (g->wi[k] + g->wo[k]) / (REAL)2;
    {
        REAL lh = SQRT_R(FN(dot3)(hs, hs));
        for (k = 0; k < 3; ++k)
            g->h[k] = hs[k] / lh;
    }
    {
        REAL VH = FN(maxr)(FN(dot3)(g->wo, g->h), (REAL)0.001f);
        g->p = POW_R((REAL)1 - VH, (REAL)5);
    }
    g->fall = (REAL)1 / (ll * ll);
}

/* map-dependent part of render(): fills ctx and returns radiance[3] */
static inline void FN(shade)(const FN(geom_t) *g, const float *col,
                             const REAL *n, const REAL *d, const REAL *rhat,
                             const REAL *s, REAL *rad, FN(ctx_t) *c)
{
    int k;
    REAL NH2, VN2, LN2, q4;
    c->nh_raw = FN(dot3)(n, g->h);
    c->vn_raw = FN(dot3)(g->wo, n);
    c->ln_raw = FN(dot3)(g->wi, n);
    c->NH = FN(maxr)(c->nh_raw, (REAL)0.001f);
    c->VN = FN(maxr)(c->vn_raw, (REAL)0.001f);
    c->LN = FN(maxr)(c->ln_raw, (REAL)0.001f);
    c->LNp = FN(maxr)(c->ln_raw, (REAL)0);
    NH2 = c->NH * c->NH;
    VN2 = c->VN * c->VN;
    LN2 = c->LN * c->LN;
    c->uV = ((REAL)1 - VN2) / VN2;
    c->uL = ((REAL)1 - LN2) / LN2;
    q4 = ((REAL)4 * c->VN) * c->LN;
    for (k = 0; k < 3; ++k) {
        REAL a, A, tV, tL, inner, den, fg, diff;
        c->r[k] = FN(maxr)(rhat[k], (REAL)0.001f);
        a = c->r[k] * c->r[k];
        A = a * a;
        c->A[k] = A;
        /* Fresnel: s + (1-s)*p */
        c->F[k] = s[k] + ((REAL)1 - s[k]) * g->p;
        /* Smith G1: 2 / (1 + sqrt(1 + (A*(1-XN^2))/XN^2)) */
        tV = (A * ((REAL)1 - VN2)) / VN2;
        tL = (A * ((REAL)1 - LN2)) / LN2;
        c->wV[k] = SQRT_R((REAL)1 + tV);
        c->wL[k] = SQRT_R((REAL)1 + tL);
        c->G1V[k] = (REAL)2 / ((REAL)1 + c->wV[k]);
        c->G1L[k] = (REAL)2 / ((REAL)1 + c->wL[k]);
        /* GGX D */
        inner = A + ((REAL)1 - NH2) / NH2;
        c->den_raw[k] = NH2 * inner;
        den = FN(maxr)(c->den_raw[k], (REAL)0.001f);
        c->den[k] = den;
        c->D[k] = A / (PI_R * (den * den));
        /* specular = F*G*D / (4*VN*LN) */
        fg = c->F[k] * (c->G1V[k] * c->G1L[k]);
        c->spec[k] = (fg * c->D[k]) / q4;
        diff = (((REAL)1 - c->F[k]) * d[k]) / PI_R;
        c->f[k] = diff + c->spec[k];
        c->E[k] = (REAL)col[k] * g->fall;
        rad[k] = (c->f[k] * c->E[k]) * c->LNp;
    }
}

/* adjoint of shade(): g_rad[3] -> accumulates into gn, gd, gr, gs */
static inline void FN(shade_bwd)(const FN(geom_t) *g, const FN(ctx_t) *c,
                                 const REAL *d, const REAL *rhat,
                                 const REAL *g_rad,
                                 REAL *gn, REAL *gd, REAL *gr, REAL *gs)
{
    int k;
    REAL g_LNp = 0, g_NH = 0, g_VN = 0, g_LN = 0, cn[3];
    const REAL q4 = ((REAL)4 * c->VN) * c->LN;
    const REAL NH2 = c->NH * c->NH;
    for (k = 0; k < 3; ++k) {
        REAL g_f = g_rad[k] * c->E[k] * c->LNp;
        REAL G = c->G1V[k] * c->G1L[k];
        REAL gdq = G * c->D[k] / q4;
        REAL g_F = g_f * (gdq - d[k] / PI_R);
        REAL g_G = g_f * c->F[k] * c->D[k] / q4;
        REAL g_D = g_f * c->F[k] * G / q4;
        REAL g_spec_over = g_f * c->spec[k];
        REAL g_G1V = g_G * c->G1L[k], g_G1L = g_G * c->G1V[k];
        REAL g_tV = -g_G1V * c->G1V[k] * c->G1V[k] / ((REAL)4 * c->wV[k]);
        REAL g_tL = -g_G1L * c->G1L[k] * c->G1L[k] / ((REAL)4 * c->wL[k]);
        REAL den = c->den[k];
        REAL g_A = g_tV * c->uV + g_tL * c->uL + g_D / (PI_R * den * den);
        REAL g_den = (c->den_raw[k] >= (REAL)0.001f)
                   ? -(REAL)2 * g_D * c->A[k] / (PI_R * den * den * den) : (REAL)0;
        g_LNp += g_rad[k] * c->f[k] * c->E[k];
        gd[k] += g_f * ((REAL)1 - c->F[k]) / PI_R;
        gs[k] += g_F * ((REAL)1 - g->p);
        /* t = A*(1/XN^2 - 1): dt/dXN = -2A/XN^3 */
        g_VN += g_tV * (-(REAL)2 * c->A[k] / (c->VN * c->VN * c->VN)) - g_spec_over / c->VN;
        g_LN += g_tL * (-(REAL)2 * c->A[k] / (c->LN * c->LN * c->LN)) - g_spec_over / c->LN;
        /* den_raw = m*(A+(1-m)/m), m = NH^2: d/dA = m, d/dm = A-1 */
        g_A += g_den * NH2;
        g_NH += g_den * (c->A[k] - (REAL)1) * (REAL)2 * c->NH;
        if (rhat[k] >= (REAL)0.001f)
            gr[k] += g_A * (REAL)4 * c->r[k] * c->r[k] * c->r[k];
    }
    if (!(c->nh_raw >= (REAL)0.001f)) g_NH = 0;
    if (!(c->vn_raw >= (REAL)0.001f)) g_VN = 0;
    if (!(c->ln_raw >= (REAL)0.001f)) g_LN = 0;
    if (!(c->ln_raw >= (REAL)0)) g_LNp = 0;
    for (k = 0; k < 3; ++k) {
        cn[k] = g_NH * g->h[k] + g_VN * g->wo[k] + (g_LN + g_LNp) * g->wi[k];
        gn[k] += cn[k];
    }
}

static inline void FN(load_maps)(const float *m, size_t plane, size_t pix,
                                 REAL *n, REAL *d, REAL *r, REAL *s)
{
    /* utils.py:40-58 unpack_svbrdf: channel order n[0:3] d[3:6] r[6:9] s[9:12] */
    int k;
    for (k = 0; k < 3; ++k) {
        n[k] = (REAL)m[(size_t)(0 + k) * plane + pix];
        d[k] = (REAL)m[(size_t)(3 + k) * plane + pix];
        r[k] = (REAL)m[(size_t)(6 + k) * plane + pix];
        s[k] = (REAL)m[(size_t)(9 + k) * plane + pix];
    }
}

/* ---- whole-tensor drivers ------------------------------------------- */

static int FN(render_fwd)(const float *maps, const float *scenes, const float *xrow,
                          OUT_T *out, int B, int S, int H, int W)
{
    const size_t plane = (size_t)H * W;
    long bi;
#pragma omp parallel for schedule(static)
    for (bi = 0; bi < (long)B * H; ++bi) {
        int b = (int)(bi / H), i = (int)(bi % H), j, sidx, k;
        const float *m = maps + (size_t)b * 12 * plane;
        REAL y = -(REAL)xrow[i];
        for (j = 0; j < W; ++j) {
            size_t pix = (size_t)i * W + j;
            REAL n[3], d[3], r[3], s[3], rad[3];
            FN(load_maps)(m, plane, pix, n, d, r, s);
            for (sidx = 0; sidx < S; ++sidx) {
                const float *sc = scenes + ((size_t)b * S + sidx) * 9;
                FN(geom_t) g;
                FN(ctx_t) c;
                FN(geometry)(sc, (REAL)xrow[j], y, &g);
                FN(shade)(&g, sc + 6, n, d, r, s, rad, &c);
                for (k = 0; k < 3; ++k)
                    out[(((size_t)b * S + sidx) * 3 + k) * plane + pix] = (OUT_T)rad[k];
            }
        }
    }
    return 0;
}

static int FN(render_bwd)(const float *maps, const float *scenes, const float *xrow,
                          const float *grad_out, OUT_T *grad_maps,
                          int B, int S, int H, int W)
{
    const size_t plane = (size_t)H * W;
    long bi;
#pragma omp parallel for schedule(static)
    for (bi = 0; bi < (long)B * H; ++bi) {
        int b = (int)(bi / H), i = (int)(bi % H), j, sidx, k;
        const float *m = maps + (size_t)b * 12 * plane;
        REAL y = -(REAL)xrow[i];
        for (j = 0; j < W; ++j) {
            size_t pix = (size_t)i * W + j;
            REAL n[3], d[3], r[3], s[3], rad[3];
            REAL gn[3] = {0, 0, 0}, gd[3] = {0, 0, 0}, gr[3] = {0, 0, 0}, gs[3] = {0, 0, 0};
            FN(load_maps)(m, plane, pix, n, d, r, s);
            for (sidx = 0; sidx < S; ++sidx) {
                const float *sc = scenes + ((size_t)b * S + sidx) * 9;
                FN(geom_t) g;
                FN(ctx_t) c;
                REAL g_rad[3];
                FN(geometry)(sc, (REAL)xrow[j], y, &g);
                FN(shade)(&g, sc + 6, n, d, r, s, rad, &c);
                for (k = 0; k < 3; ++k)
                    g_rad[k] = (REAL)grad_out[(((size_t)b * S + sidx) * 3 + k) * plane + pix];
                FN(shade_bwd)(&g, &c, d, r, g_rad, gn, gd, gr, gs);
            }
            for (k = 0; k < 3; ++k) {
                OUT_T *gm = grad_maps + (size_t)b * 12 * plane + pix;
                gm[(size_t)(0 + k) * plane] = (OUT_T)gn[k];
                gm[(size_t)(3 + k) * plane] = (OUT_T)gd[k];
                gm[(size_t)(6 + k) * plane] = (OUT_T)gr[k];
                gm[(size_t)(9 + k) * plane] = (OUT_T)gs[k];
            }
        }
    }
    return 0;
}

/* losses.py:29-52 with the scenes given explicitly ([B,S,9]); with l1_weight != 0 also
 * losses.py:7-19 (SVBRDFL1Loss: L1 of normals and roughness, L1 of log(x+eps_l1) for
 * diffuse and specular, each a mean over B*3*H*W) combined as in losses.py:62-63
 * (MixedLoss = l1_weight * L1 + rendering).
 * input_lo (optional, [B,12,H,W]): added to the input maps after their conversion to REAL -- the low parts of maps that
 * are not float32 values (the double instantiation of the head-fused loss decodes the head in double).
 * tie_allow (optional, [B,12,H,W]): per gradient element, 2 * sum over the pixel's tied terms -- those the tie map
 * counts (not a structural zero) with |delta| < tie_level -- of |that term's sign-free contribution| (shade_bwd of
 * g_rad = invN / ai in its one channel).  Where sign(delta) is rounding noise an fp32 evaluation may pick either sign
 * (or 0), which moves the gradient by at most that much.  The L1 part never adds to it. */
static int FN(rendering_loss)(const float *input, const double *input_lo, const float *target,
                              const float *scenes, const float *xrow, float eps,
                              float l1_weight, float eps_l1,
                              double *loss_out, OUT_T *grad_input, OUT_T *min_abs_delta,
                              OUT_T *tie_allow, double tie_level,
                              int B, int S, int H, int W)
{
    const size_t plane = (size_t)H * W;
    const double N = (double)B * S * 3 * (double)plane;
    const double NL = (double)B * 3 * (double)plane;
    const REAL invN = (REAL)(1.0 / N);
    const REAL wl = (REAL)((double)l1_weight / NL);
    double total = 0.0, total_l1 = 0.0;
    long bi;
#pragma omp parallel for schedule(static) reduction(+ : total, total_l1)
    for (bi = 0; bi < (long)B * H; ++bi) {
        int b = (int)(bi / H), i = (int)(bi % H), j, sidx, k;
        const float *mi = input + (size_t)b * 12 * plane;
        const float *mt = target + (size_t)b * 12 * plane;
        REAL y = -(REAL)xrow[i];
        double rowsum = 0.0, rowl1 = 0.0;
        for (j = 0; j < W; ++j) {
            size_t pix = (size_t)i * W + j;
            REAL n[3], d[3], r[3], s[3], tn[3], td[3], tr[3], ts[3];
            REAL gn[3] = {0, 0, 0}, gd[3] = {0, 0, 0}, gr[3] = {0, 0, 0}, gs[3] = {0, 0, 0};
            REAL tie = (REAL)1e30;      /* smallest |log difference| of this pixel: sign() is noise below ~1e-6 */
            REAL al[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   /* tie allowance of the 12 gradient elements */
            FN(load_maps)(mi, plane, pix, n, d, r, s);
            if (input_lo) {     /* the input maps are input + input_lo: maps decoded in double (head_loss, f64) */
                const double *lo = input_lo + (size_t)b * 12 * plane + pix;
                for (k = 0; k < 3; ++k) {
                    n[k] += (REAL)lo[(size_t)(0 + k) * plane];
                    d[k] += (REAL)lo[(size_t)(3 + k) * plane];
                    r[k] += (REAL)lo[(size_t)(6 + k) * plane];
                    s[k] += (REAL)lo[(size_t)(9 + k) * plane];
                }
            }
            FN(load_maps)(mt, plane, pix, tn, td, tr, ts);
            if (l1_weight != 0.0f) {
                for (k = 0; k < 3; ++k) {
                    REAL dn = n[k] - tn[k], dr = r[k] - tr[k];
                    REAL dd = LOG_R(d[k] + (REAL)eps_l1) - LOG_R(td[k] + (REAL)eps_l1);
                    REAL ds = LOG_R(s[k] + (REAL)eps_l1) - LOG_R(ts[k] + (REAL)eps_l1);
                    rowl1 += (double)(dn < 0 ? -dn : dn) + (double)(dr < 0 ? -dr : dr)
                           + (double)(dd < 0 ? -dd : dd) + (double)(ds < 0 ? -ds : ds);
                    gn[k] = wl * (dn > 0 ? (REAL)1 : (dn < 0 ? (REAL)-1 : (REAL)0));
                    gr[k] = wl * (dr > 0 ? (REAL)1 : (dr < 0 ? (REAL)-1 : (REAL)0));
                    gd[k] = wl * (dd > 0 ? (REAL)1 : (dd < 0 ? (REAL)-1 : (REAL)0)) / (d[k] + (REAL)eps_l1);
                    gs[k] = wl * (ds > 0 ? (REAL)1 : (ds < 0 ? (REAL)-1 : (REAL)0)) / (s[k] + (REAL)eps_l1);
                }
            }
            for (sidx = 0; sidx < S; ++sidx) {
                const float *sc = scenes + ((size_t)b * S + sidx) * 9;
                FN(geom_t) g;
                FN(ctx_t) ci, ct;
                REAL ri[3], rt[3], g_rad[3];
                FN(geometry)(sc, (REAL)xrow[j], y, &g);
                FN(shade)(&g, sc + 6, n, d, r, s, ri, &ci);
                FN(shade)(&g, sc + 6, tn, td, tr, ts, rt, &ct);
                for (k = 0; k < 3; ++k) {
                    REAL ai = ri[k] + (REAL)eps, at = rt[k] + (REAL)eps;
                    REAL delta = LOG_R(ai) - LOG_R(at);
                    REAL sg = delta > 0 ? (REAL)1 : (delta < 0 ? (REAL)-1 : (REAL)0);
                    rowsum += (double)(delta < 0 ? -delta : delta);
                    /* structural zero: both renderings are exactly 0 because the light is clearly below
                     * both surfaces' horizon (LN+ clamp) -- sign(0) = 0 in every implementation */
                    int structural = ci.ln_raw < (REAL)-1e-6 && ct.ln_raw < (REAL)-1e-6;
                    if (!structural)
                        if ((delta < 0 ? -delta : delta) < tie) tie = (delta < 0 ? -delta : delta);
                    g_rad[k] = sg * invN / ai;
                    if (tie_allow && !structural && (double)(delta < 0 ? -delta : delta) < tie_level) {
                        REAL one[3] = {0, 0, 0}, z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                        int e;
                        one[k] = invN / ai;
                        FN(shade_bwd)(&g, &ci, d, r, one, z, z + 3, z + 6, z + 9);
                        for (e = 0; e < 12; ++e)
                            al[e] += z[e] < 0 ? -z[e] : z[e];
                    }
                }
                if (grad_input)
                    FN(shade_bwd)(&g, &ci, d, r, g_rad, gn, gd, gr, gs);
            }
            if (min_abs_delta) min_abs_delta[(size_t)b * plane + pix] = (OUT_T)tie;
            if (tie_allow)
                for (k = 0; k < 12; ++k)
                    tie_allow[(size_t)b * 12 * plane + (size_t)k * plane + pix] = (OUT_T)((REAL)2 * al[k]);
            if (grad_input) {
                OUT_T *gm = grad_input + (size_t)b * 12 * plane + pix;
                for (k = 0; k < 3; ++k) {
                    gm[(size_t)(0 + k) * plane] = (OUT_T)gn[k];
                    gm[(size_t)(3 + k) * plane] = (OUT_T)gd[k];
                    gm[(size_t)(6 + k) * plane] = (OUT_T)gr[k];
                    gm[(size_t)(9 + k) * plane] = (OUT_T)gs[k];
                }
            }
        }
        total += rowsum;
        total_l1 += rowl1;
    }
    *loss_out = total / N + (double)l1_weight * (total_l1 / NL);
    return 0;
}

#undef PI_R
