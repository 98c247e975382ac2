/* The adjoint arbiter (oracle/rr_oracle_adj.c) on tiny networks, as a program of its own: built by tests/test_adjoint_oracle.py with
 * AddressSanitizer and UndefinedBehaviorSanitizer and run there.  Every array is allocated at its exact size, so a read or a write one
 * element beyond any of them stops the program.  Each case runs both precisions, with and without each optional argument, and checks
 * that the two agree to 1e-12 of an element's scale and that a scale is never below the magnitude of its gradient. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef int rapid_fn(int64_t, const int32_t *, const int32_t *, const double *, const double *, const double *, const double *,
                     const double *, const double *, const double *, const double *, int64_t, int64_t,
                     double *, double *, double *, double *, double *, double *, double *);
typedef int unit_fn(int64_t, const int32_t *, const int32_t *, const double *, const double *, const double *,
                    const double *, const double *, const double *, const double *, const double *, const double *, int64_t, int64_t,
                    double *, double *, double *, double *, double *, double *, double *, double *);
rapid_fn orc_rapid_adjoint, orcl_rapid_adjoint;
unit_fn orc_unit_adjoint, orcl_unit_adjoint;

static uint64_t rng_state = 88172645463325252ull;
static double u01(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}
static double *filled(size_t count, double lo, double hi)
{
    double *a = (double *)malloc(sizeof(double) * (count ? count : 1));
    if (!a) exit(3);
    for (size_t i = 0; i < count; ++i) a[i] = lo + (hi - lo) * u01();
    return a;
}
static int failures;
static void compare(const char *what, const double *a, const double *b, const double *scale, size_t count)
{
    for (size_t i = 0; i < count; ++i) {
        if (!(scale[i] >= fabs(b[i]))) { printf("FAIL %s[%zu]: scale %g below |gradient| %g\n", what, i, scale[i], fabs(b[i])); ++failures; return; }
        if (fabs(a[i] - b[i]) > 1e-12 * scale[i]) { printf("FAIL %s[%zu]: %.17g against %.17g at scale %g\n", what, i, a[i], b[i], scale[i]); ++failures; return; }
    }
}

/* down[i] >= 0: the reach i flows into (> i); -1 at an outlet.  variant bit 0: no lateral (Rapid only), 1: no dL/ddischarge, 2: no final-state cotangents */
static void run_case(const char *name, int64_t n, const int64_t *down, int64_t T, int64_t nsub, int variant)
{
    int32_t *indptr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
    int64_t edges = 0, n_inner = 0;
    for (int64_t i = 0; i < n; ++i) edges += down[i] >= 0;
    int32_t *indices = (int32_t *)malloc(sizeof(int32_t) * (size_t)(edges ? edges : 1));
    char *inner = (char *)calloc((size_t)n, 1);
    if (!indptr || !indices || !inner) exit(3);
    indptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        indptr[i + 1] = indptr[i];
        if (down[i] >= 0) { indices[indptr[i + 1]++] = (int32_t)down[i]; inner[down[i]] = 1; }
    }
    for (int64_t i = 0; i < n; ++i) n_inner += inner[i];
    const size_t N = (size_t)n, TN = (size_t)(T * n), NI = (size_t)n_inner;
    double *c1 = filled(N, 0.05, 0.4), *c2 = filled(N, 0.1, 0.5), *c3 = filled(N, -0.3, 0.5), *c4 = filled(N, 1e-4, 3e-4);
    double *q0 = filled(N, 0.0, 3.0), *ql = filled(TN, -2000.0, 7000.0), *G = filled(TN, -1.0, 1.0), *Gf = filled(N, -1.0, 1.0);
    double *qc0 = filled(NI, 0.0, 80.0), *qf0 = filled(NI, 0.0, 120.0), *Gc = filled(NI, -1.0, 1.0), *Gff = filled(NI, -1.0, 1.0);
    const double *lat = (variant & 1) ? NULL : ql, *g = (variant & 2) ? NULL : G, *gf = (variant & 4) ? NULL : Gf;
    double *out[2][7];
    for (int p = 0; p < 2; ++p) {
        out[p][0] = filled(4 * N, 0, 0); out[p][1] = filled(N, 0, 0); out[p][2] = filled(TN, 0, 0);
        out[p][3] = filled(4 * N, 0, 0); out[p][4] = filled(N, 0, 0); out[p][5] = filled(TN, 0, 0); out[p][6] = filled(TN, 0, 0);
        rapid_fn *f = p ? orcl_rapid_adjoint : orc_rapid_adjoint;
        const int rc = f(n, indptr, indices, c1, c2, c3, c4, q0, lat, g, gf, T, nsub, out[p][0], out[p][1], lat ? out[p][2] : NULL,
                         out[p][3], out[p][4], lat ? out[p][5] : NULL, out[p][6]);
        if (rc) { printf("FAIL %s: rapid adjoint returned %d\n", name, rc); ++failures; }
    }
    compare("rapid grad_coef", out[0][0], out[1][0], out[1][3], 4 * N);
    compare("rapid grad_q0", out[0][1], out[1][1], out[1][4], N);
    if (lat) compare("rapid grad_lateral", out[0][2], out[1][2], out[1][5], TN);
    for (int p = 0; p < 2; ++p) for (int k = 0; k < 7; ++k) free(out[p][k]);

    double *uo[2][8];
    for (int p = 0; p < 2; ++p) {
        uo[p][0] = filled(3 * N, 0, 0); uo[p][1] = filled(NI, 0, 0); uo[p][2] = filled(NI, 0, 0); uo[p][3] = filled(TN, 0, 0);
        uo[p][4] = filled(3 * N, 0, 0); uo[p][5] = filled(2 * NI, 0, 0); uo[p][6] = filled(TN, 0, 0); uo[p][7] = filled(TN, 0, 0);
        unit_fn *f = p ? orcl_unit_adjoint : orc_unit_adjoint;
        const int rc = f(n, indptr, indices, c1, c2, c3, qc0, qf0, ql, g, (variant & 4) ? NULL : Gc, (variant & 4) ? NULL : Gff, T, nsub,
                         uo[p][0], uo[p][1], uo[p][2], uo[p][3], uo[p][4], uo[p][5], uo[p][6], uo[p][7]);
        if (rc) { printf("FAIL %s: unit adjoint returned %d\n", name, rc); ++failures; }
    }
    compare("unit grad_coef", uo[0][0], uo[1][0], uo[1][4], 3 * N);
    compare("unit grad_qch0", uo[0][1], uo[1][1], uo[1][5], NI);
    compare("unit grad_qfull0", uo[0][2], uo[1][2], uo[1][5] + NI, NI);
    compare("unit grad_lateral", uo[0][3], uo[1][3], uo[1][6], TN);
    for (int p = 0; p < 2; ++p) for (int k = 0; k < 8; ++k) free(uo[p][k]);
    free(c1); free(c2); free(c3); free(c4); free(q0); free(ql); free(G); free(Gf); free(qc0); free(qf0); free(Gc); free(Gff);
    free(indptr); free(indices); free(inner);
    printf("%s (variant %d): done\n", name, variant);
}

int main(void)
{
    const int64_t one[] = {-1}, lone[] = {-1, -1, -1, -1}, star[] = {5, 5, 5, 5, 5, -1}, chain[] = {1, 2, 3, 4, -1};
    const int64_t tree[] = {4, 4, 5, 5, 6, 6, 8, 8, -1, 10, -1};      /* two outlets, a headwater into each level */
    for (int variant = 0; variant < 8; ++variant) {
        run_case("one reach", 1, one, 3, 2, variant);
        run_case("no edges", 4, lone, 2, 3, variant);
        run_case("star", 6, star, 4, 1, variant);
        run_case("chain", 5, chain, 5, 3, variant);
        run_case("tree", 11, tree, 7, 2, variant);
    }
    /* the refusals: a downstream index outside the network, a reach that flows upstream */
    {
        const int32_t indptr[] = {0, 1, 1}, far[] = {7}, back_ptr[] = {0, 0, 1}, back[] = {0};
        double z[16] = {0}, o[8][16];
        if (orc_rapid_adjoint(2, indptr, far, z, z, z, z, z, z, z, z, 2, 1, o[0], o[1], o[2], o[3], o[4], o[5], o[6]) != -3) { puts("FAIL: -3 expected"); ++failures; }
        if (orcl_unit_adjoint(2, back_ptr, back, z, z, z, z, z, z, z, z, z, 2, 1, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]) != -4) { puts("FAIL: -4 expected"); ++failures; }
    }
    if (failures) { printf("adjoint oracle: %d failures\n", failures); return 1; }
    puts("adjoint oracle: all cases ok");
    return 0;
}
