/*
 * r2s_oracle.c - CPU restatement of the Rho2sdf.jl hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product path (rho2sdf.jl_amd/,
 * include/) may include, link or call this file; only tests/, bench.py's
 * cpu_baseline leg and __graft_entry__.smoke() use it, as the checker.
 *
 * It restates, function by function, what the Julia reference computes
 * (citations are paths under /root/reference).  Plain scalar C, single
 * thread, written in the reference's own loop structure (element-major
 * scatter through the point->cell linked list), which is deliberately NOT
 * the structure of the HIP kernels (voxel-major gather over tile bins).
 *
 * Third-party arithmetic that is absent from /root/reference:
 *   - NLopt 2.10.0 LD_SLSQP  (ComputeCoordsOnIso.jl:19-86): the constrained
 *     closest-point problem is restated (objective, constraint, bounds,
 *     start point) and solved to tight tolerance by the SQP documented at
 *     iso_project_hex8() below.  PARITY UNPINNED for curved iso-surfaces
 *     beyond the reference's own known answers (tests/golden) and an
 *     independent SLSQP (scipy's Kraft SLSQP) cross-check.
 *   - NLopt LD_LBFGS (FindLocalCoordinates.jl:71-106): bounded inverse
 *     isoparametric map; restated as a box-clamped Newton iteration.
 *   - LAPACK eigen / LU: restated as cyclic Jacobi / partial-pivot LU.
 *
 * Compile with -ffp-contract=off: every expression that feeds an integer or
 * boolean decision keeps the reference's operation order and must not be
 * contracted into FMAs.
 */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BIG 1.0e10

typedef struct {
    double amin[3];
    double amax[3];
    int64_t N[3];
    double cell;
    int64_t ngp;
} orc_grid;

/* ------------------------------------------------------------------ */
/* Grid  (src/MeshGrid/Grid.jl:10-34)                                  */
/* ------------------------------------------------------------------ */
int orc_grid_make(const double xmin[3], const double xmax[3], int64_t n_max,
                  int64_t margin, orc_grid *g)
{
    double ext = xmax[0] - xmin[0];
    for (int i = 1; i < 3; ++i)
        if (xmax[i] - xmin[i] > ext) ext = xmax[i] - xmin[i];
    double cell = ext / (double)n_max;                 /* Grid.jl:17 */
    double m = (double)margin * cell;
    g->ngp = 1;
    for (int i = 0; i < 3; ++i) {
        double lo = xmin[i] - m;                       /* Grid.jl:20 */
        double hi = xmax[i] + m;                       /* Grid.jl:21 */
        g->N[i] = (int64_t)ceil((hi - lo) / cell);     /* Grid.jl:24 */
        g->amin[i] = lo;
        g->amax[i] = lo + (double)g->N[i] * cell;      /* Grid.jl:26 */
        g->ngp *= g->N[i] + 1;                         /* Grid.jl:30 */
    }
    g->cell = cell;
    return 0;
}

/* grid point i,j,k  (Grid.jl:87: AABB_min .+ cell_size .* [i,j,k]) */
static inline void grid_point(const orc_grid *g, int64_t i, int64_t j, int64_t k, double p[3])
{
    p[0] = g->amin[0] + g->cell * (double)i;
    p[1] = g->amin[1] + g->cell * (double)j;
    p[2] = g->amin[2] + g->cell * (double)k;
}

/* cell index of a coordinate (Grid.jl:58, :134-135): floor(N*(x-min)/(max-min)) */
static inline double cell_of(const orc_grid *g, int ax, double x)
{
    return floor((double)g->N[ax] * (x - g->amin[ax]) / (g->amax[ax] - g->amin[ax]));
}

void orc_grid_points(const orc_grid *g, double *pts /* 3*ngp */)
{
    int64_t a = 0;
    for (int64_t k = 0; k <= g->N[2]; ++k)
        for (int64_t j = 0; j <= g->N[1]; ++j)
            for (int64_t i = 0; i <= g->N[0]; ++i, ++a)
                grid_point(g, i, j, k, pts + 3 * a);
}

/* ------------------------------------------------------------------ */
/* Element tables  (src/ElementTypes/ElementTypes.jl:15-78)            */
/* ------------------------------------------------------------------ */
static const int HEX_ISN[6][4] = {{0, 3, 2, 1}, {0, 1, 5, 4}, {1, 2, 6, 5},
                                  {2, 3, 7, 6}, {3, 0, 4, 7}, {4, 5, 6, 7}};
static const int TET_ISN[4][3] = {{0, 2, 1}, {0, 1, 3}, {1, 2, 3}, {0, 3, 2}};
static const int HEX_EDGES[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6},
                                     {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
static const int TET_EDGES[6][2] = {{0, 1}, {1, 2}, {2, 0}, {0, 3}, {1, 3}, {2, 3}};

/* ------------------------------------------------------------------ */
/* Shape functions (src/ShapeFunctions/hex8_shape.jl:2-70)             */
/* ------------------------------------------------------------------ */
static void hex8_shape(const double xi[3], double N[8])
{
    double x1m = xi[0] - 1, x1p = xi[0] + 1, x2m = xi[1] - 1, x2p = xi[1] + 1;
    double x3m = xi[2] - 1, x3p = xi[2] + 1;
    double t1 = x1m * x2m, t2 = x1p * x2m, t3 = x1p * x2p, t4 = x1m * x2p;
    const double c = 0.125;
    N[0] = -c * t1 * x3m;
    N[1] = c * t2 * x3m;
    N[2] = -c * t3 * x3m;
    N[3] = c * t4 * x3m;
    N[4] = c * t1 * x3p;
    N[5] = -c * t2 * x3p;
    N[6] = c * t3 * x3p;
    N[7] = -c * t4 * x3p;
}

static void hex8_shape_d(const double xi[3], double N[8], double dN[8][3])
{
    double x1m = xi[0] - 1, x1p = xi[0] + 1, x2m = xi[1] - 1, x2p = xi[1] + 1;
    double x3m = xi[2] - 1, x3p = xi[2] + 1;
    double t1 = x1m * x2m, t2 = x1p * x2m, t3 = x1p * x2p, t4 = x1m * x2p;
    const double c = 0.125;
    N[0] = -c * t1 * x3m;
    N[1] = c * t2 * x3m;
    N[2] = -c * t3 * x3m;
    N[3] = c * t4 * x3m;
    N[4] = c * t1 * x3p;
    N[5] = -c * t2 * x3p;
    N[6] = c * t3 * x3p;
    N[7] = -c * t4 * x3p;
    double d1 = c * x3m, d1p = c * x3p;
    dN[0][0] = -d1 * x2m;  dN[1][0] = d1 * x2m;   dN[2][0] = -d1 * x2p;  dN[3][0] = d1 * x2p;
    dN[4][0] = d1p * x2m;  dN[5][0] = -d1p * x2m; dN[6][0] = d1p * x2p;  dN[7][0] = -d1p * x2p;
    dN[0][1] = -d1 * x1m;  dN[1][1] = d1 * x1p;   dN[2][1] = -d1 * x1p;  dN[3][1] = d1 * x1m;
    dN[4][1] = d1p * x1m;  dN[5][1] = -d1p * x1p; dN[6][1] = d1p * x1p;  dN[7][1] = -d1p * x1m;
    dN[0][2] = -c * t1;    dN[1][2] = c * t2;     dN[2][2] = -c * t3;    dN[3][2] = c * t4;
    dN[4][2] = c * t1;     dN[5][2] = -c * t2;    dN[6][2] = c * t3;     dN[7][2] = -c * t4;
}

/* mixed second derivatives of the trilinear shape functions (pure ones are 0);
 * m[k][0] = d2N/dxi1 dxi2, m[k][1] = d2N/dxi1 dxi3, m[k][2] = d2N/dxi2 dxi3 */
static void hex8_shape_mixed(const double xi[3], double m[8][3])
{
    static const double sg[8] = {-1, 1, -1, 1, 1, -1, 1, -1};
    double x1[2] = {xi[0] - 1, xi[0] + 1}, x2[2] = {xi[1] - 1, xi[1] + 1};
    double x3[2] = {xi[2] - 1, xi[2] + 1};
    static const int s1[8] = {0, 1, 1, 0, 0, 1, 1, 0};
    static const int s2[8] = {0, 0, 1, 1, 0, 0, 1, 1};
    static const int s3[8] = {0, 0, 0, 0, 1, 1, 1, 1};
    for (int k = 0; k < 8; ++k) {
        double c = 0.125 * sg[k];
        m[k][0] = c * x3[s3[k]];
        m[k][1] = c * x2[s2[k]];
        m[k][2] = c * x1[s1[k]];
    }
}

/* ------------------------------------------------------------------ */
/* small dense helpers                                                 */
/* ------------------------------------------------------------------ */
static inline double norm3(const double v[3])
{
    return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

/* n x n LU with partial pivoting (stands in for LAPACK getrf/getrs behind
 * Julia's `\`); returns 0 on success, 1 if singular. */
static int lu_solve(int n, double *A /* n*n row-major, destroyed */, double *b)
{
    for (int c = 0; c < n; ++c) {
        int p = c;
        double best = fabs(A[c * n + c]);
        for (int r = c + 1; r < n; ++r)
            if (fabs(A[r * n + c]) > best) { best = fabs(A[r * n + c]); p = r; }
        if (best == 0.0) return 1;
        if (p != c) {
            for (int k = 0; k < n; ++k) { double t = A[c * n + k]; A[c * n + k] = A[p * n + k]; A[p * n + k] = t; }
            double t = b[c]; b[c] = b[p]; b[p] = t;
        }
        for (int r = c + 1; r < n; ++r) {
            double l = A[r * n + c] / A[c * n + c];
            A[r * n + c] = l;
            for (int k = c + 1; k < n; ++k) A[r * n + k] -= l * A[c * n + k];
            b[r] -= l * b[c];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double s = b[r];
        for (int k = r + 1; k < n; ++k) s -= A[r * n + k] * b[k];
        b[r] = s / A[r * n + r];
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* Monomial form of the trilinear maps (solver internals only)         */
/*   X(xi) = sum_m C[m] mono_m(xi),                                     */
/*   mono = [1, x1, x2, x3, x1x2, x1x3, x2x3, x1x2x3]                    */
/* The coefficients live behind the nodal values: Xe[8+m], re[8+m]      */
/* (element arrays are declared with 16 rows).  The reference evaluates */
/* N(xi) node by node (hex8_shape.jl); the restated solvers (NLopt      */
/* stand-ins) use this cheaper, algebraically identical form, while     */
/* every quantity the reference itself computes (xp = Xe N, rho = N.re) */
/* keeps the nodal form.                                                */
/* ------------------------------------------------------------------ */
static const double MONO_SIGN[8][8] = {
    /* node:      0   1   2   3   4   5   6   7 */
    /* 1     */ { 1,  1,  1,  1,  1,  1,  1,  1},
    /* x1    */ {-1,  1,  1, -1, -1,  1,  1, -1},
    /* x2    */ {-1, -1,  1,  1, -1, -1,  1,  1},
    /* x3    */ {-1, -1, -1, -1,  1,  1,  1,  1},
    /* x1x2  */ { 1, -1,  1, -1,  1, -1,  1, -1},
    /* x1x3  */ { 1, -1, -1,  1, -1,  1,  1, -1},
    /* x2x3  */ { 1,  1, -1, -1, -1, -1,  1,  1},
    /* x1x2x3*/ {-1,  1, -1,  1,  1, -1,  1, -1}};

static void hex8_monomials(double Xe[16][3], double re[16])
{
    for (int m = 0; m < 8; ++m) {
        for (int i = 0; i < 3; ++i) {
            double t = 0.0;
            for (int k = 0; k < 8; ++k) t += MONO_SIGN[m][k] * Xe[k][i];
            Xe[8 + m][i] = 0.125 * t;
        }
        double t = 0.0;
        for (int k = 0; k < 8; ++k) t += MONO_SIGN[m][k] * re[k];
        re[8 + m] = 0.125 * t;
    }
}

/* value and first derivatives of one scalar trilinear field with coefficients c[0..7] (stride st) */
/* a0 b0 + a1 b1 + a2 b2 with a fixed fused evaluation order (one multiply, two FMAs) */
static inline double dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return fma(a2, b2, fma(a1, b1, a0 * b0));
}

typedef struct { double v, d1, d2, d3, m12, m13, m23; } tri_eval;
static inline tri_eval tri_eval_full(const double *c, int st, const double xi[3])
{
    tri_eval o;
    double q0 = fma(xi[2], c[3 * st], c[0]);          /* C0 + C3 x3    */
    double q1 = fma(xi[2], c[5 * st], c[1 * st]);     /* C1 + C13 x3   */
    double q2 = fma(xi[2], c[6 * st], c[2 * st]);     /* C2 + C23 x3   */
    double q3 = fma(xi[2], c[7 * st], c[4 * st]);     /* C12 + C123 x3 */
    double r0 = fma(xi[1], q2, q0);
    double r1 = fma(xi[1], q3, q1);                   /* d/dx1         */
    o.v = fma(xi[0], r1, r0);
    o.d1 = r1;
    o.d2 = fma(xi[0], q3, q2);
    o.m13 = fma(xi[1], c[7 * st], c[5 * st]);         /* C13 + C123 x2 */
    o.m23 = fma(xi[0], c[7 * st], c[6 * st]);         /* C23 + C123 x1 */
    o.d3 = fma(xi[0], o.m13, fma(xi[1], c[6 * st], c[3 * st]));
    o.m12 = q3;
    return o;
}
static inline double tri_eval_value(const double *c, int st, const double xi[3])
{
    double q0 = fma(xi[2], c[3 * st], c[0]);
    double q1 = fma(xi[2], c[5 * st], c[1 * st]);
    double q2 = fma(xi[2], c[6 * st], c[2 * st]);
    double q3 = fma(xi[2], c[7 * st], c[4 * st]);
    return fma(xi[0], fma(xi[1], q3, q1), fma(xi[1], q2, q0));
}

/* ------------------------------------------------------------------ */
/* Inverse isoparametric map, HEX8                                     */
/* (src/SignedDistances/FindLocalCoordinates.jl:16-107)                */
/*                                                                     */
/* Reference: min ||Xe N(xi) - x||^2 over the box [-1.1,1.1]^3 with    */
/* NLopt L-BFGS from 9 starts.  Restated as Newton on Xe N(xi) = x     */
/* from xi = 0 with every iterate clamped to the same box: a root      */
/* inside the box is found to machine precision; when the root lies    */
/* outside the iterate sticks to the box boundary (max|xi| = 1.1),      */
/* which every caller rejects (thresholds 1.001 / 1.01), exactly as it  */
/* rejects the reference's boundary minimiser.  Non-convergence returns */
/* (10,10,10) like the reference's failure path (:106).                */
/* ------------------------------------------------------------------ */
/* -DORC_TIGHT builds the FROZEN tight-tolerance variant (libr2s_oracle_tight.so): same algorithm, step
 * tolerances 1e-13 / 1e-12 and generous iteration caps.  tests/test_oracle_drift.py holds the production
 * tolerances below against it on every fixture, so that an edit which trades accuracy for speed shows up as
 * a number instead of passing silently ("freeze the oracle"). */
#ifdef ORC_TIGHT
#define INV_MAXIT 200
#else
#define INV_MAXIT 50
#endif
/* Step tolerance: Newton converges quadratically here, so the iterate AFTER a step below 1e-7 is within ~1e-14
 * of the root - the accuracy a 1e-10 tolerance delivers, one iteration earlier (the last iteration of that rule
 * only confirms a step of ~1e-15).  The reference's own optimiser stops at xtol_rel 1e-6 / ftol_abs 1e-10
 * (FindLocalCoordinates.jl:79-87). */
#ifdef ORC_TIGHT
#define INV_TOL 1e-13
#else
#define INV_TOL 1e-7
#endif
static int inv_map_hex8(const double Xe[16][3] /* nodes + monomials */, const double x[3], double xi[3])
{
    xi[0] = xi[1] = xi[2] = 0.0;
    for (int it = 0; it < INV_MAXIT; ++it) {
        double R[3], J[3][3];
        for (int i = 0; i < 3; ++i) {
            tri_eval t = tri_eval_full(&Xe[8][i], 3, xi);
            R[i] = t.v - x[i];
            J[i][0] = t.d1; J[i][1] = t.d2; J[i][2] = t.d3;
        }
        /* delta = -J^{-1} R by the adjugate; every a*b - c*d is fma(a, b, -(c*d)), sums of three
         * products are dot3: the GPU kernels perform the identical IEEE operations */
        double c00 = fma(J[1][1], J[2][2], -(J[1][2] * J[2][1]));
        double c01 = fma(J[1][2], J[2][0], -(J[1][0] * J[2][2]));
        double c02 = fma(J[1][0], J[2][1], -(J[1][1] * J[2][0]));
        double det = dot3(J[0][0], J[0][1], J[0][2], c00, c01, c02);
        double c10 = fma(J[0][2], J[2][1], -(J[0][1] * J[2][2]));
        double c11 = fma(J[0][0], J[2][2], -(J[0][2] * J[2][0]));
        double c12 = fma(J[0][1], J[2][0], -(J[0][0] * J[2][1]));
        double c20 = fma(J[0][1], J[1][2], -(J[0][2] * J[1][1]));
        double c21 = fma(J[0][2], J[1][0], -(J[0][0] * J[1][2]));
        double c22 = fma(J[0][0], J[1][1], -(J[0][1] * J[1][0]));
        double rdet = 1.0 / det;
        double d0 = -dot3(c00, c10, c20, R[0], R[1], R[2]) * rdet;
        double d1 = -dot3(c01, c11, c21, R[0], R[1], R[2]) * rdet;
        double d2 = -dot3(c02, c12, c22, R[0], R[1], R[2]) * rdet;
        double n0 = fmin(fmax(xi[0] + d0, -1.1), 1.1);
        double n1 = fmin(fmax(xi[1] + d1, -1.1), 1.1);
        double n2 = fmin(fmax(xi[2] + d2, -1.1), 1.1);
        double step = fmax(fabs(n0 - xi[0]), fmax(fabs(n1 - xi[1]), fabs(n2 - xi[2])));
        xi[0] = n0; xi[1] = n1; xi[2] = n2;
        if (!(step > INV_TOL)) {
            if (step != step) break; /* NaN: degenerate element */
            return 1;
        }
    }
    xi[0] = xi[1] = xi[2] = 10.0;
    return 0;
}

/* find_local_coordinates for one (element, point): tests compare it with 9-start L-BFGS-B vectors */
int orc_inv_map_hex8(const double x[3], const double *Xe_flat /* 8*3 */, double xi[3])
{
    double Xe[16][3], re[16] = {0};
    for (int a = 0; a < 8; ++a)
        for (int i = 0; i < 3; ++i) Xe[a][i] = Xe_flat[3 * a + i];
    hex8_monomials(Xe, re);
    return inv_map_hex8(Xe, x, xi);
}

/* ------------------------------------------------------------------ */
/* Projection onto the density iso-surface inside one HEX8             */
/* (src/SignedDistances/ComputeCoordsOnIso.jl:16-87)                   */
/*                                                                     */
/*   min_xi ||x - Xe N(xi)||^2  s.t.  N(xi).rho_e = rho_t, -1<=xi<=1    */
/*   start xi = 0 (ComputeCoordsOnIso.jl:25-26,70,78)                  */
/*                                                                     */
/* Reference optimiser: NLopt LD_SLSQP (tolerances 1e-5, maxeval 1000).  Restated as a second-order SQP on the same
 * problem from the same start, converged to ISO_TOL on a step of the convex mode (DESIGN.md section 2 has the reasons
 * for every rule and what round 2's version got wrong):
 *   - Hessian of the Lagrangian: always the exact one (Gauss-Newton part 2 J^T J plus the mixed second derivatives of
 *     the trilinear maps, multiplier = least squares over the free variables), convexified along the constraint
 *     normal (H + sigma a a^T, two sizes of sigma);
 *   - convex on the faces the active-set walk visits: QP (3 unknowns, 1 linear equality, box cut with the trust region)
 *     solved exactly - walk from the previous pattern, exhaustive search over the 19 patterns when it cycles; L1 merit
 *     f + mu |c| with back-tracking and a second-order correction at the first failed trial;
 *   - not convex: global minimiser of the QP over box and trust region, taken as a trust-region step (actual against
 *     predicted reduction of the merit function), the region shrinks on rejection;
 *   - linearised equality out of reach inside the trust region: step to the corner that comes closest; out of reach
 *     anywhere in the element, or no descent off the surface: restoration along the segments to the nodes on the other
 *     side of rho_t;
 *   - rounding residue of the density field (1e-14 of its scale) counts as zero; a constraint gradient without a
 *     component along the free variables makes the equality vacuous on that face;
 *   - failing runs (caps, Brent's cycle test) return the nearest iterate that was on the iso-surface.                  */
/* ------------------------------------------------------------------ */
#define ISO_MAXIT 100
#define ISO_MAX_NONCONVEX 48 /* iterations on a non-convex model per run: converging runs were seen to need <= 30 (<= 47 iterations in
                                all); runs beyond that go round in not-quite-periodic cycles on nearly degenerate elements */
/* Step tolerance.  The iteration ends AFTER applying a step below it, and only a step of the CONVEX mode (exact
 * Lagrangian Hessian positive definite on the face the QP ends on) may end it: those steps shrink quadratically, so
 * the final iterate is within ~tol^2 of the minimiser.  (Round 2 also ended on small Gauss-Newton steps, which
 * converge linearly - up to 1000 x the step away from the limit - and towards saddle points.)  The reference stops
 * its SLSQP at xtol_rel = ftol_rel = 1e-5 (ComputeCoordsOnIso.jl:20-22). */
#ifdef ORC_TIGHT
#define ISO_TOL 1e-12
#else
#define ISO_TOL 1e-6
#endif
#define QP_PTOL 1e-12
#define ISO_MAX_RESTORE 3
#define MU_FEAS 1e10 /* x rtol = 1e-4 of the density scale */

typedef struct {
    double f, c;
} iso_fc;

static inline iso_fc iso_eval_fc(const double x[3], const double Xe[16][3], const double re[16],
                                 double rt, const double xi[3])
{
    iso_fc o;
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = x[i] - tri_eval_value(&Xe[8][i], 3, xi);
    double rho = tri_eval_value(&re[8], 1, xi);
    o.f = dot3(r[0], r[1], r[2], r[0], r[1], r[2]);
    o.c = rho - rt;
    return o;
}

/* one active-set pattern of the QP; returns 1 if primal feasible */
static int qp_pattern(int pat, const double H[3][3], const double g[3], const double a[3],
                      double e, const double lo[3], const double hi[3], double d[3],
                      double *lam_out, double *q_out, int *kkt_out, int *next_pat)
{
    /* returns 0: pattern unusable (the matrix is not positive definite on this face: its stationary point is no
     * minimiser), 2: primal infeasible, 1: primal feasible (kkt_out tells optimality);
     * next_pat: the pattern an active-set step would try next (fix the most violated free variable /
     * release the fixed variable with the worst multiplier), -1 if none */
    static const int pw[3] = {1, 3, 9};
    *next_pat = -1;
    int s[3] = {pat % 3, (pat / 3) % 3, pat / 9};
    double dB[3], aa[3], b[3], M[3][3];
    for (int i = 0; i < 3; ++i) dB[i] = (s[i] == 1) ? lo[i] : ((s[i] == 2) ? hi[i] : 0.0);
    double ep = e;
    for (int i = 0; i < 3; ++i) {
        if (s[i]) {
            ep = fma(-a[i], dB[i], ep);
            aa[i] = 0.0;
            b[i] = 0.0;
        } else {
            aa[i] = a[i];
            double t = -g[i];
            for (int j = 0; j < 3; ++j)
                if (s[j]) t = fma(-H[i][j], dB[j], t);
            b[i] = t;
        }
        for (int j = 0; j < 3; ++j)
            M[i][j] = (s[i] || s[j]) ? ((i == j) ? 1.0 : 0.0) : H[i][j];
    }
    /* inverse of the masked symmetric matrix by its adjugate (one division); the leading minors
     * double as the positive-definiteness test (Sylvester) */
    const double M00 = M[0][0], M01 = M[0][1], M02 = M[0][2], M11 = M[1][1], M12 = M[1][2], M22 = M[2][2];
    const double c00 = fma(M11, M22, -(M12 * M12));
    const double c01 = fma(M02, M12, -(M01 * M22));
    const double c02 = fma(M01, M12, -(M02 * M11));
    const double c11 = fma(M00, M22, -(M02 * M02));
    const double c12 = fma(M01, M02, -(M00 * M12));
    const double c22 = fma(M00, M11, -(M01 * M01));
    const double det = dot3(M00, M01, M02, c00, c01, c02);
    if (!(M00 > 0.0 && c22 > 0.0 && det > 0.0)) return 0;
    const double rdet = 1.0 / det;
    double u[3], v[3];
    u[0] = dot3(c00, c01, c02, aa[0], aa[1], aa[2]) * rdet;
    u[1] = dot3(c01, c11, c12, aa[0], aa[1], aa[2]) * rdet;
    u[2] = dot3(c02, c12, c22, aa[0], aa[1], aa[2]) * rdet;
    v[0] = dot3(c00, c01, c02, b[0], b[1], b[2]) * rdet;
    v[1] = dot3(c01, c11, c12, b[0], b[1], b[2]) * rdet;
    v[2] = dot3(c02, c12, c22, b[0], b[1], b[2]) * rdet;
    double den = dot3(aa[0], aa[1], aa[2], u[0], u[1], u[2]);
    /* vacuous equality: the constraint gradient has no component along the free variables (rho is constant on this
     * face of the element - an iso-surface that coincides with an element face, as on 0/1 density fields).  The face
     * problem is then unconstrained if the fixed variables meet the equality, infeasible otherwise. */
    const int vac = (aa[0] == 0.0 && aa[1] == 0.0 && aa[2] == 0.0);
    if (vac ? (ep != 0.0) : !(den > 0.0)) return 0;
    double lam = vac ? 0.0 : (dot3(aa[0], aa[1], aa[2], v[0], v[1], v[2]) - ep) / den;
    int ok = 1;
    double worst = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (s[i]) {
            d[i] = dB[i];
        } else {
            d[i] = fma(-lam, u[i], v[i]);
            if (!(d[i] >= lo[i] - QP_PTOL && d[i] <= hi[i] + QP_PTOL)) {
                ok = 0;
                double below = (lo[i] - QP_PTOL) - d[i], above = d[i] - (hi[i] + QP_PTOL);
                double viol = fmax(below, above);
                if (viol > worst) { worst = viol; *next_pat = pat + ((above > below) ? 2 : 1) * pw[i]; }
            }
        }
    }
    if (!ok) {
        /* two variables fixed already: fixing the violated third one leaves no freedom for the
         * equality, so the walk restarts from the violated bound alone */
        const int np = *next_pat;
        if (np >= 0 && (np % 3) && ((np / 3) % 3) && (np / 9)) {
            for (int i = 0; i < 3; ++i)
                if (!s[i]) *next_pat = ((np / pw[i]) % 3) * pw[i];
        }
        return 2;
    }
    double Hd[3], q = 0.0;
    for (int i = 0; i < 3; ++i) {
        Hd[i] = dot3(H[i][0], H[i][1], H[i][2], d[0], d[1], d[2]);
        q = fma(d[i], fma(0.5, Hd[i], g[i]), q);
    }
    int kkt = 1;
    worst = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (s[i] && !(vac && a[i] != 0.0)) { /* (vacuous equality: its multiplier is free and absorbs z) */
            double z = fma(lam, a[i], Hd[i] + g[i]);
            double viol = (s[i] == 1) ? -z : z;
            if (s[i] == 1 && !(z >= 0.0)) kkt = 0;
            if (s[i] == 2 && !(z <= 0.0)) kkt = 0;
            if (viol > worst) { worst = viol; *next_pat = pat - s[i] * pw[i]; }
        }
    }
    *lam_out = lam;
    *q_out = q;
    *kkt_out = kkt;
    return 1;
}

static int spd3(const double H[3][3], double floor_)
{
    /* Sylvester's criterion on the (symmetric) matrix: leading minors, no division */
    const double c00 = fma(H[1][1], H[2][2], -(H[1][2] * H[1][2]));
    const double c01 = fma(H[0][2], H[1][2], -(H[0][1] * H[2][2]));
    const double c02 = fma(H[0][1], H[1][2], -(H[0][2] * H[1][1]));
    const double m2 = fma(H[0][0], H[1][1], -(H[0][1] * H[0][1]));
    const double det = dot3(H[0][0], H[0][1], H[0][2], c00, c01, c02);
    return (H[0][0] > floor_) && (m2 > floor_) && (det > floor_);
}

/* per-call statistics of the solver (research / tests: orc_iso_project_hex8_batch) */
typedef struct {
    int it, nonconvex, corner, restore, backtrack, reject, code; /* code 1: converged, 2: flat, 3: failed */
} iso_stats;
static iso_stats g_iso_stats;

/* Restoration: the linearised constraint cannot be met anywhere in the element (|xi| <= 1), so first-order steps
 * cannot reach the iso-surface from here (it only clips a corner region of the element, or the density has a saddle at
 * the iterate).  An iso element has nodes on either side of the threshold; along the straight segment from the iterate
 * to a node k on the OTHER side, rho - rho_t (a cubic in the segment parameter) changes sign, so the segment holds a
 * feasible point: bracketed Newton finds the first root for every such node and the candidate with the smallest
 * distance to x becomes the new iterate (ties: lowest node).  Returns 0 if no node lies on the other side. */
static int iso_restore(const double x[3], const double Xe[16][3], const double re[16], double rt,
                       const double xi[3], double c, double out[3])
{
    double bestf = INFINITY;
    int found = 0;
    for (int k = 0; k < 8; ++k) {
        const double nd[3] = {(k & 1) ? 1.0 : -1.0, (k & 2) ? 1.0 : -1.0, (k & 4) ? 1.0 : -1.0};
        const double ck = tri_eval_value(&re[8], 1, nd) - rt;
        if ((c < 0.0) ? !(ck >= 0.0) : !(ck <= 0.0)) continue;
        const double dir[3] = {nd[0] - xi[0], nd[1] - xi[1], nd[2] - xi[2]};
        /* phi(t) = rho(xi + t dir) - rt, phi(0) = c, phi(1) = ck: signs differ (or ck = 0) */
        double tl = 0.0, th = 1.0, t = 1.0, p[3] = {nd[0], nd[1], nd[2]};
        if (ck != 0.0) {
            t = 0.5;
            for (int n = 0; n < 100; ++n) {
                for (int i = 0; i < 3; ++i) p[i] = fma(t, dir[i], xi[i]);
                const tri_eval tr = tri_eval_full(&re[8], 1, p);
                const double ph = tr.v - rt;
                if (ph == 0.0) break;
                if ((ph < 0.0) == (c < 0.0)) tl = t; else th = t;
                if (!(th - tl > 1e-15)) break;
                const double dph = dot3(tr.d1, tr.d2, tr.d3, dir[0], dir[1], dir[2]);
                double tn = t - ph / dph;
                if (!(tn > tl && tn < th)) tn = 0.5 * (tl + th);
                if (tn == t) break;
                t = tn;
            }
            for (int i = 0; i < 3; ++i) p[i] = fmin(fmax(fma(t, dir[i], xi[i]), -1.0), 1.0);
        }
        const iso_fc fc = iso_eval_fc(x, Xe, re, rt, p);
        if (fc.f < bestf) { bestf = fc.f; found = 1; out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; }
    }
    return found;
}

/* returns number of iterations used (ISO_MAXIT+1 if not converged) */
static int iso_project_hex8(const double x[3], const double Xe[16][3], const double re[16], double rt, double xi[3]);
int orc_iso_project_hex8(const double x[3], const double *Xe_flat /* 8*3 */, const double re_in[8],
                         double rt, double xi[3])
{
    double Xe[16][3], re[16];
    for (int k = 0; k < 8; ++k) {
        for (int i = 0; i < 3; ++i) Xe[k][i] = Xe_flat[3 * k + i];
        re[k] = re_in[k];
    }
    hex8_monomials(Xe, re);
    return iso_project_hex8(x, Xe, re, rt, xi);
}

/* n independent (point, element) problems; stats: 7 ints per problem (iso_stats) or NULL */
void orc_iso_project_hex8_batch(int64_t n, const double *x /* n*3 */, const double *Xe_flat /* n*8*3 */,
                                const double *re_in /* n*8 */, const double *rt /* n */, double *xi /* n*3 */,
                                int *stats /* n*7 or NULL */)
{
    for (int64_t p = 0; p < n; ++p) {
        orc_iso_project_hex8(x + 3 * p, Xe_flat + 24 * p, re_in + 8 * p, rt[p], xi + 3 * p);
        if (stats) memcpy(stats + 7 * p, &g_iso_stats, sizeof(iso_stats));
    }
}

/* the solver proper; Xe/re carry the monomial coefficients in rows 8..15 */
static int iso_project_hex8(const double x[3], const double Xe[16][3], const double re[16], double rt, double xi[3])
{
    xi[0] = xi[1] = xi[2] = 0.0;
    double mu = 0.0, lam = 0.0, Delta = 2.0;
    int pat = 0, nrest = 0;
    iso_stats st = {0, 0, 0, 0, 0, 0, 3};
    double rtol = fabs(rt);
    for (int k = 0; k < 8; ++k) rtol = fmax(rtol, fabs(re[k]));
    rtol *= 1e-14;
    double fbest = INFINITY, xbest[3] = {0.0, 0.0, 0.0};
    double sx[3] = {0.0, 0.0, 0.0}, smu = -1.0, sDelta = -1.0; /* cycle detection: state at iteration 16, 32, 64, 128 */
    int spat = -1;
    for (int it = 0; it < ISO_MAXIT; ++it) {
        double r[3], J[3][3], a[3], g[3], G[3][3], M2[3][3]; /* M2[i][q]: mixed derivatives of p_i */
        /* The iteration is a deterministic map of (xi, mu, Delta, pattern): a state that comes back will come back for
         * ever (nearly degenerate elements - an iso-surface within 1e-4 of an element face - send feasibility steps,
         * restorations and QP steps round in cycles of period 3-9).  Brent's scheme: remember the state at iterations
         * 16, 32, 64, 128 and stop as failed when it recurs, instead of running to the cap (the slowest lane sets the
         * run time of the device's straggler launch). */
        if (it > 16 && xi[0] == sx[0] && xi[1] == sx[1] && xi[2] == sx[2] && mu == smu && Delta == sDelta && pat == spat) {
            st.it = it; g_iso_stats = st;
            if (fbest < INFINITY) { xi[0] = xbest[0]; xi[1] = xbest[1]; xi[2] = xbest[2]; }
            return ISO_MAXIT + 1;
        }
        if (it == 16 || it == 32 || it == 64 || it == 128) {
            sx[0] = xi[0]; sx[1] = xi[1]; sx[2] = xi[2]; smu = mu; sDelta = Delta; spat = pat;
        }
        for (int i = 0; i < 3; ++i) {
            tri_eval t = tri_eval_full(&Xe[8][i], 3, xi);
            r[i] = x[i] - t.v;
            J[i][0] = t.d1; J[i][1] = t.d2; J[i][2] = t.d3;
            M2[i][0] = t.m12; M2[i][1] = t.m13; M2[i][2] = t.m23;
        }
        const double f = dot3(r[0], r[1], r[2], r[0], r[1], r[2]);
        tri_eval tr = tri_eval_full(&re[8], 1, xi);
        double c = tr.v - rt;
        a[0] = tr.d1; a[1] = tr.d2; a[2] = tr.d3;
        /* rounding residue of the density field counts as zero: a constraint value or a gradient component of
         * ~1e-16 (an iso-surface that runs along an element face) must not decide corner steps or multipliers */
        if (fabs(c) <= rtol) c = 0.0;
        for (int j = 0; j < 3; ++j)
            if (fabs(a[j]) <= rtol) a[j] = 0.0;
        /* the nearest iterate ON the iso-surface so far: what a run that fails hands back */
        if (c == 0.0 && f < fbest) { fbest = f; xbest[0] = xi[0]; xbest[1] = xi[1]; xbest[2] = xi[2]; }
        for (int j = 0; j < 3; ++j) g[j] = -2.0 * dot3(r[0], r[1], r[2], J[0][j], J[1][j], J[2][j]);
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j)
                G[i][j] = G[j][i] = 2.0 * dot3(J[0][i], J[1][i], J[2][i], J[0][j], J[1][j], J[2][j]);
        /* warm-start pattern: a variable the last QP fixed stays fixed only if it sits on the element's own bound
         * now (a bound of the trust region says nothing about the next QP) */
        {
            const int s[3] = {pat % 3, (pat / 3) % 3, pat / 9};
            pat = 0;
            if ((s[0] == 1 && xi[0] == -1.0) || (s[0] == 2 && xi[0] == 1.0)) pat += s[0];
            if ((s[1] == 1 && xi[1] == -1.0) || (s[1] == 2 && xi[1] == 1.0)) pat += 3 * s[1];
            if ((s[2] == 1 && xi[2] == -1.0) || (s[2] == 2 && xi[2] == 1.0)) pat += 9 * s[2];
        }
        /* multiplier estimate for the Hessian: least squares over the variables
         * that were free in the last QP solution */
        {
            double num = 0.0, den = 0.0;
            int s[3] = {pat % 3, (pat / 3) % 3, pat / 9};
            for (int i = 0; i < 3; ++i)
                if (!s[i]) { num = fma(a[i], g[i], num); den = fma(a[i], a[i], den); }
            lam = (den > 0.0) ? -num / den : 0.0;
        }
        /* second-order part: S_jl = -2 sum_i r_i d2p_i/djdl + lam d2rho/djdl */
        double S[3]; /* (0,1) (0,2) (1,2) */
        {
            const double mr[3] = {tr.m12, tr.m13, tr.m23};
            for (int q = 0; q < 3; ++q)
                S[q] = fma(lam, mr[q], -2.0 * dot3(r[0], r[1], r[2], M2[0][q], M2[1][q], M2[2][q]));
        }
        double lo[3], hi[3], d[3];
        for (int i = 0; i < 3; ++i) {
            lo[i] = fmax(-1.0 - xi[i], -Delta);
            hi[i] = fmin(1.0 - xi[i], Delta);
        }
        double e = -c, mplus = 0.0, mminus = 0.0;
        for (int i = 0; i < 3; ++i) {
            double p = a[i] * lo[i], q = a[i] * hi[i];
            mplus += fmax(p, q);
            mminus += fmin(p, q);
        }
        double trG = G[0][0] + G[1][1] + G[2][2];
        double aa2 = dot3(a[0], a[1], a[2], a[0], a[1], a[2]);
        double sigma = 100.0 * trG / aa2;
        int convex = 1, corner = 0, stop = 0, stall = 0;
        /* the penalty parameter of the merit function may shrink (towards twice the multiplier) only where the
         * constraint is nearly met (|rho - rho_t| <= 1e-4 of the density scale): halving it at infeasible iterates let a
         * step that trades feasibility for distance undo the feasibility step before it (2-cycles between a box corner and
         * the point it was reached from); never letting it shrink left runs that had needed a large parameter once
         * crawling along the iso-surface in trust-region-sized steps (26 -> 19 iterations on the north-star family) */
        const int near_feas = (fabs(c) <= 1e4 * rtol);
        const double mu_keep = (fabs(c) <= MU_FEAS * rtol) ? 0.5 : 1.0;
        double lam_new = lam, alpha = 1.0, qstep = 0.0;
        double dGd = 0.0; /* curvature of f along a corner step (penalty parameter below) */
        if (e > mplus) {
            for (int i = 0; i < 3; ++i) d[i] = (a[i] > 0.0) ? hi[i] : ((a[i] < 0.0) ? lo[i] : 0.0);
            corner = 1;
        } else if (e < mminus) {
            for (int i = 0; i < 3; ++i) d[i] = (a[i] > 0.0) ? lo[i] : ((a[i] < 0.0) ? hi[i] : 0.0);
            corner = 1;
        }
        if (corner) {
            /* how much of the constraint violation the linear model can remove anywhere in the element: next to
             * nothing means that first-order steps are stuck (the density has a stationary point here or the
             * iso-surface only clips a corner region the gradient does not point to) - straight to the restoration.
             * The test does not depend on the stopping tolerance. */
            double bp = 0.0, bm = 0.0;
            for (int i = 0; i < 3; ++i) {
                const double p = a[i] * (-1.0 - xi[i]), q = a[i] * (1.0 - xi[i]);
                bp += fmax(p, q);
                bm += fmin(p, q);
            }
            if ((e > 0.0) ? !(bp > 0.05 * e) : !(bm < 0.05 * e)) stall = 1;
            double Gd[3];
            for (int i = 0; i < 3; ++i) Gd[i] = dot3(G[i][0], G[i][1], G[i][2], d[0], d[1], d[2]);
            dGd = dot3(d[0], d[1], d[2], Gd[0], Gd[1], Gd[2]);
        } else {
            /* QP data with the EXACT Lagrangian Hessian, convexified along the constraint normal:
             * H = G + S + sigma a a^T, g' = g - sigma e a (identical to (G + S, g) on the plane a.d = e; positive
             * definite on a face of the box exactly when G + S is positive definite on that face cut with the plane,
             * provided sigma is large enough).  sigma = 100 tr(G) / |a|^2 first; where the matrix is not positive
             * definite with it the test is repeated with 100 times that before the model is declared non-convex
             * (weak constraint gradients - an iso-surface close to an element face - come with large multipliers, and
             * then lam d2rho outgrows 100 tr(G)). */
            double H[3][3], gp[3];
            int stage = 0;
            double sg = sigma;
            for (;;) {
                const double se = sg * e;
                for (int i = 0; i < 3; ++i) {
                    const double sa = sg * a[i];
                    for (int j = i; j < 3; ++j) H[i][j] = H[j][i] = fma(sa, a[j], G[i][j]);
                    gp[i] = fma(-se, a[i], g[i]);
                }
                H[0][1] += S[0]; H[1][0] = H[0][1];
                H[0][2] += S[1]; H[2][0] = H[0][2];
                H[1][2] += S[2]; H[2][1] = H[1][2];
                /* convex mode while the matrix is positive definite on the faces the active-set walk visits, starting
                 * with the face of the box the last QP ended on (warm-start pattern) */
                double Hm[3][3];
                const int sp[3] = {pat % 3, (pat / 3) % 3, pat / 9};
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) Hm[i][j] = (sp[i] || sp[j]) ? ((i == j) ? 1.0 : 0.0) : H[i][j];
                convex = spd3(Hm, 0.0);
                if (convex || stage) break;
                stage = 1;
                sg = 100.0 * sigma;
            }
            double q, dd[3], l2;
            int kkt, found = 0, nxt;
            if (convex) {
                /* active-set walk from the previous pattern: the first pattern that is primal
                 * feasible and satisfies KKT is the minimiser of the QP when it is convex on the faces seen */
                int p = pat;
                for (int step = 0; step < 8 && p >= 0; ++step) {
                    int rc = qp_pattern(p, H, gp, a, e, lo, hi, dd, &l2, &q, &kkt, &nxt);
                    if (rc == 0 && !stage) {
                        /* the walk left the warm-start face for one on which the matrix is not positive definite:
                         * once more with the larger sigma, from the warm-start pattern */
                        stage = 1;
                        sg = 100.0 * sigma;
                        const double se = sg * e;
                        for (int i = 0; i < 3; ++i) {
                            const double sa = sg * a[i];
                            for (int j = i; j < 3; ++j) H[i][j] = H[j][i] = fma(sa, a[j], G[i][j]);
                            gp[i] = fma(-se, a[i], g[i]);
                        }
                        H[0][1] += S[0]; H[1][0] = H[0][1];
                        H[0][2] += S[1]; H[2][0] = H[0][2];
                        H[1][2] += S[2]; H[2][1] = H[1][2];
                        p = pat;
                        step = -1;
                        continue;
                    }
                    if (rc == 0) { convex = 0; break; }
                    if (rc == 1 && kkt) {
                        found = 1;
                        pat = p;
                        d[0] = dd[0]; d[1] = dd[1]; d[2] = dd[2];
                        lam_new = l2;
                        qstep = q;
                        break;
                    }
                    p = nxt;
                }
            }
            if (!found) {
                /* exhaustive search over the patterns with 0, 1, 2 fixed variables (3 fixed cannot meet the
                 * equality).  Convex: first KKT pattern, failing that (rounding) the feasible one of least value.
                 * Not convex: the stationary points of the faces on which the matrix is positive definite (the
                 * others are no minimisers of their face: the minimum then lies on the face's boundary, which the
                 * patterns with one more fixed variable cover) - the one of least value is the global minimiser of
                 * the QP over the box cut with the trust region. */
                static const int order[19] = {0, 1, 2, 3, 6, 9, 18, 4, 5, 7, 8,
                                              10, 11, 19, 20, 12, 15, 21, 24};
                double bestq = INFINITY;
                for (int ip = 0; ip < 19; ++ip) {
                    const int p = order[ip];
                    if (qp_pattern(p, H, gp, a, e, lo, hi, dd, &l2, &q, &kkt, &nxt) == 1) {
                        if ((convex && kkt) || q < bestq) {
                            bestq = q;
                            found = 1;
                            pat = p;
                            d[0] = dd[0]; d[1] = dd[1]; d[2] = dd[2];
                            lam_new = l2;
                            qstep = q;
                        }
                        if (convex && kkt) break;
                    }
                }
            }
            if (!found) { /* numerically degenerate: corner move towards feasibility */
                for (int i = 0; i < 3; ++i)
                    d[i] = (e > 0.0) ? ((a[i] > 0.0) ? hi[i] : ((a[i] < 0.0) ? lo[i] : 0.0))
                                     : ((a[i] > 0.0) ? lo[i] : ((a[i] < 0.0) ? hi[i] : 0.0));
                corner = 1;
                convex = 1;
            }
            for (int i = 0; i < 3; ++i) d[i] = fmin(fmax(d[i], lo[i]), hi[i]);
        }
        st.corner += corner;
        st.nonconvex += !convex;
        if (st.nonconvex > ISO_MAX_NONCONVEX) {
            st.it = it + 1; g_iso_stats = st;
            if (fbest < INFINITY) { xi[0] = xbest[0]; xi[1] = xbest[1]; xi[2] = xbest[2]; }
            return ISO_MAXIT + 1;
        }
        const double dmax = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2])));
        const double ad = dot3(a[0], a[1], a[2], d[0], d[1], d[2]);
        const double pred_c = fabs(c) - fabs(c + ad);
        if (stall) {
            stop = 2;
        } else if (!convex) {
            /* Trust-region step of the non-convex model (negative curvature of the Lagrangian along the iso-surface:
             * the iterate is near a saddle point or a maximum of the distance).  One trial at the full step, accepted
             * on actual against predicted reduction of the L1 merit function; a rejected step shrinks the region. */
            double mu_t = fmax(mu_keep * mu, 2.0 * fabs(lam_new));
            double pred = fma(mu_t, pred_c, -qstep);
            if (!(pred > 0.0)) {
                if (pred_c > 0.0) { mu_t = 2.0 * qstep / pred_c; pred = qstep; }
                else stop = near_feas ? 3 : 2; /* feasible and the model offers no decrease: second-order point */
            }
            if (!stop && !(pred > 1e-14 * f)) stop = 3; /* no negative curvature worth a step: second-order point */
            if (!stop) {
                mu = mu_t;
                double xt[3];
                for (int i = 0; i < 3; ++i) xt[i] = fmin(fmax(xi[i] + d[i], -1.0), 1.0);
                iso_fc t = iso_eval_fc(x, Xe, re, rt, xt);
                const double phi0 = fma(mu, fabs(c), f);
                if (!(phi0 - fma(mu, fabs(t.c), t.f) >= 1e-4 * pred)) {
                    /* second-order correction (see the convex mode below), then rejection */
                    const int sp[3] = {pat % 3, (pat / 3) % 3, pat / 9};
                    double den = 0.0, d2[3] = {d[0], d[1], d[2]};
                    int ok = 0;
                    for (int i = 0; i < 3; ++i)
                        if (!sp[i]) den = fma(a[i], a[i], den);
                    if (den > 0.0) {
                        const double sc = -t.c / den;
                        for (int i = 0; i < 3; ++i) {
                            if (!sp[i]) d2[i] = fma(sc, a[i], d[i]);
                            xt[i] = fmin(fmax(xi[i] + d2[i], -1.0), 1.0);
                        }
                        iso_fc t2 = iso_eval_fc(x, Xe, re, rt, xt);
                        ok = (phi0 - fma(mu, fabs(t2.c), t2.f) >= 1e-4 * pred);
                    }
                    if (ok) { d[0] = d2[0]; d[1] = d2[1]; d[2] = d2[2]; }
                    else { alpha = 0.0; st.reject++; }
                }
            }
        } else if (!(dmax > ISO_TOL)) { /* converged (a feasible vertex of the box counts), or stuck at an infeasible corner */
            stop = (corner && !near_feas) ? 2 : 1;
        } else {
            double gd = dot3(g[0], g[1], g[2], d[0], d[1], d[2]);
            double mu_t = corner ? mu : fmax(mu_keep * mu, 2.0 * fabs(lam_new));
            if (corner && pred_c > 0.0) {
                /* The linearised constraint cannot be met inside the trust region: the step only buys
                 * feasibility, and the merit function has to pay for the growth of f it causes including its
                 * curvature (mu >= (g.d + d.G.d / 2) / ((1 - 1/2) pred_c), Nocedal & Wright (18.36)). */
                const double need = 2.0 * fma(0.5, dGd, gd) / pred_c;
                if (need > mu_t) mu_t = need;
            }
            if (!(fma(-mu_t, pred_c, gd) < 0.0)) {
                if (pred_c > 0.0) mu_t = 2.0 * gd / pred_c;
                else stop = (near_feas && !corner) ? 4 : 2; /* no descent on the merit function; from a feasible
                                                            * point: the QP step is rounding noise - converged */
            }
            if (!stop) {
                mu = mu_t;
                double D = fma(-mu, pred_c, gd);
                double phi0 = fma(mu, fabs(c), f);
                for (int ls = 0; ls < 30; ++ls) {
                    double xt[3];
                    for (int i = 0; i < 3; ++i) xt[i] = fmin(fmax(fma(alpha, d[i], xi[i]), -1.0), 1.0);
                    iso_fc t = iso_eval_fc(x, Xe, re, rt, xt);
                    if (fma(mu, fabs(t.c), t.f) <= fma(1e-4 * alpha, D, phi0)) break;
                    if (ls == 0 && !corner) {
                        /* second-order correction: the full step fails on the curvature of the iso-surface (the merit
                         * function sees rho leave rho_t by O(|d|^2)); the least-norm move of the free variables that
                         * cancels rho(xi + d) - rho_t to first order is added and the trial repeated (Maratos effect:
                         * without it steps along a strongly curved iso-surface shrink to ~1e-4 and crawl) */
                        const int sp[3] = {pat % 3, (pat / 3) % 3, pat / 9};
                        double den = 0.0;
                        for (int i = 0; i < 3; ++i)
                            if (!sp[i]) den = fma(a[i], a[i], den);
                        if (den > 0.0) {
                            const double sc = -t.c / den;
                            double d2[3];
                            for (int i = 0; i < 3; ++i) {
                                d2[i] = sp[i] ? d[i] : fma(sc, a[i], d[i]);
                                xt[i] = fmin(fmax(xi[i] + d2[i], -1.0), 1.0);
                            }
                            iso_fc t2 = iso_eval_fc(x, Xe, re, rt, xt);
                            if (fma(mu, fabs(t2.c), t2.f) <= fma(1e-4, D, phi0)) {
                                d[0] = d2[0]; d[1] = d2[1]; d[2] = d2[2];
                                st.reject++; /* (counted as corrected steps in convex mode) */
                                break;
                            }
                        }
                    }
                    alpha *= 0.5;
                    st.backtrack++;
                }
            }
        }
        Delta = (alpha < 1.0) ? ((alpha > 0.0) ? alpha * dmax : 0.25 * dmax) : fmin(2.0, fmax(Delta, 2.0 * dmax));
#ifdef ISO_DEBUG
        printf("it %d xi %.6f %.6f %.6f f %.3e c %.3e d %.3e %.3e %.3e alpha %.3e pat %d corner %d cvx %d lam %.3e mu %.3e stop %d\n",
               it, xi[0], xi[1], xi[2], f, c, d[0], d[1], d[2], alpha, pat, corner, convex, lam, mu, stop);
#endif
        st.it = it + 1;
        if (stop == 2) {
            /* no descent / stuck at a point that does not satisfy the constraint */
            double xr[3];
            if (!near_feas && nrest < ISO_MAX_RESTORE && iso_restore(x, Xe, re, rt, xi, c, xr)) {
                st.restore++;
                xi[0] = xr[0]; xi[1] = xr[1]; xi[2] = xr[2];
                mu = 0.0; Delta = 2.0; pat = 0; nrest++;
                continue;
            }
            g_iso_stats = st;
            if (fbest < INFINITY) { xi[0] = xbest[0]; xi[1] = xbest[1]; xi[2] = xbest[2]; }
            return ISO_MAXIT + 1;
        }
        if (stop == 3 || stop == 4) { st.code = (stop == 3) ? 2 : 1; g_iso_stats = st; return it + 1; }
        for (int i = 0; i < 3; ++i) xi[i] = fmin(fmax(fma(alpha, d[i], xi[i]), -1.0), 1.0);
        if (stop == 1) { st.code = 1; g_iso_stats = st; return it + 1; }
    }
    g_iso_stats = st;
    if (fbest < INFINITY) { xi[0] = xbest[0]; xi[1] = xbest[1]; xi[2] = xbest[2]; }
    return ISO_MAXIT + 1;
}

/* ------------------------------------------------------------------ */
/* Mesh helpers                                                        */
/* ------------------------------------------------------------------ */
typedef struct {
    const double *X;    /* [nnp][3]  (Julia 3 x nnp column-major)        */
    const int64_t *IEN; /* [nel][nen] 1-based (Julia nen x nel)          */
    int64_t nnp, nel;
    int nen, nes, nsn;
    int elem_type; /* 0 = HEX8, 1 = TET4 */
    /* node -> elements CSR (MeshInformations.jl:69-77), ascending element order */
    int64_t *ine_ptr;
    int64_t *ine;
} orc_mesh;

static int mesh_init(orc_mesh *m, const double *X, int64_t nnp, const int64_t *IEN, int64_t nel,
                     int elem_type)
{
    m->X = X; m->IEN = IEN; m->nnp = nnp; m->nel = nel; m->elem_type = elem_type;
    if (elem_type == 0) { m->nen = 8; m->nes = 6; m->nsn = 4; }
    else { m->nen = 4; m->nes = 4; m->nsn = 3; }
    m->ine_ptr = (int64_t *)calloc((size_t)nnp + 1, sizeof(int64_t));
    for (int64_t e = 0; e < nel; ++e)
        for (int a = 0; a < m->nen; ++a) {
            int64_t n = IEN[e * m->nen + a] - 1;
            if (n < 0 || n >= nnp) return -1;
            m->ine_ptr[n + 1]++;
        }
    for (int64_t n = 0; n < nnp; ++n) m->ine_ptr[n + 1] += m->ine_ptr[n];
    m->ine = (int64_t *)malloc(sizeof(int64_t) * (size_t)m->ine_ptr[nnp]);
    int64_t *cur = (int64_t *)malloc(sizeof(int64_t) * (size_t)nnp);
    memcpy(cur, m->ine_ptr, sizeof(int64_t) * (size_t)nnp);
    for (int64_t e = 0; e < nel; ++e)
        for (int a = 0; a < m->nen; ++a) {
            int64_t n = IEN[e * m->nen + a] - 1;
            m->ine[cur[n]++] = e;
        }
    free(cur);
    return 0;
}
static void mesh_free(orc_mesh *m) { free(m->ine_ptr); free(m->ine); }

static inline int face_node(const orc_mesh *m, int sg, int a)
{
    return m->elem_type == 0 ? HEX_ISN[sg][a] : TET_ISN[sg][a];
}

/* boundary test of sdfOnDensityField.jl:511-519: intersect the node->element
 * lists of the face nodes; boundary <=> exactly one common element */
static int face_is_boundary(const orc_mesh *m, int64_t el, int sg)
{
    int64_t n0 = m->IEN[el * m->nen + face_node(m, sg, 0)] - 1;
    int count = 0;
    for (int64_t p = m->ine_ptr[n0]; p < m->ine_ptr[n0 + 1]; ++p) {
        int64_t e = m->ine[p];
        int all = 1;
        for (int a = 1; a < m->nsn && all; ++a) {
            int64_t na = m->IEN[el * m->nen + face_node(m, sg, a)] - 1;
            int found = 0;
            for (int64_t q = m->ine_ptr[na]; q < m->ine_ptr[na + 1]; ++q)
                if (m->ine[q] == e) { found = 1; break; }
            all = found;
        }
        count += all;
    }
    return count == 1;
}

/* ------------------------------------------------------------------ */
/* evalDistances (src/SignedDistances/sdfOnDensityField.jl:139-486)    */
/* ------------------------------------------------------------------ */
typedef struct {
    const orc_grid *g;
    int64_t *head, *next;
    double *dist; /* running |dist_local| (sdfOnDensityField.jl:183: -1e10 -> abs) */
    double *xp;   /* [ngp][3] */
    double delta;
    int elem_type;
    /* statistics */
    int64_t n_iso_solves, n_iso_fail, n_tri_tests, n_invmap;
} dist_ctx;

/* mini AABB of a point set, as cell index ranges (Grid.jl:122-154) */
static void mini_aabb(const orc_grid *g, const double (*P)[3], int np, double delta,
                      int64_t Imin[3], int64_t Imax[3])
{
    for (int ax = 0; ax < 3; ++ax) {
        double mn = P[0][ax], mx = P[0][ax];
        for (int k = 1; k < np; ++k) {
            if (P[k][ax] < mn) mn = P[k][ax];
            if (P[k][ax] > mx) mx = P[k][ax];
        }
        double lo = cell_of(g, ax, mn - delta);
        double hi = cell_of(g, ax, mx + delta);
        if (lo < 0) lo = 0;
        if (hi >= (double)g->N[ax]) hi = (double)g->N[ax];
        Imin[ax] = (int64_t)lo;
        Imax[ax] = (int64_t)hi;
    }
}

/* WriteValue (sdfOnDensityField.jl:44-57) / update_distance_parallel! (:121-136) */
/* order-independent "true minimum" semantics (orc_set_true_min): every valid candidate of a
 * triangle takes part in the minimum (no "first improving edge wins", sdfOnDensityField.jl:769-771, no vertex
 * fall-back only after failures, :777), exact ties go to the lexicographically smaller projection point, and the
 * HEX8 sign is +1 as soon as ANY candidate element that holds the point (max|xi| < 1.01) has rho >= rho_t
 * (instead of the improving-sequence rule of SignDetection.jl:56-69).  Result: independent of element order and
 * of the thread / GPU partition; dist_true <= dist_ordered everywhere. */
static int g_true_min = 0;
void orc_set_true_min(int on) { g_true_min = on; }

static inline int write_value(dist_ctx *c, int64_t v, double d, const double xp[3])
{
    if (g_true_min && c->xp && fabs(d) == c->dist[v]) { /* symmetric tie rule */
        double *q = c->xp + 3 * v;
        int less = xp[0] < q[0] || (xp[0] == q[0] && (xp[1] < q[1] || (xp[1] == q[1] && xp[2] < q[2])));
        if (less) { q[0] = xp[0]; q[1] = xp[1]; q[2] = xp[2]; }
        return 0;
    }
    if (fabs(d) < c->dist[v]) {
        c->dist[v] = d;
        if (c->xp) { c->xp[3 * v] = xp[0]; c->xp[3 * v + 1] = xp[1]; c->xp[3 * v + 2] = xp[2]; }
        return 1;
    }
    return 0;
}

/* IsProjectedOnFullSegment, HEX8 branch (sdfOnDensityField.jl:78-119) */
static int projected_on_full_segment_hex8(dist_ctx *c, const double Xe[16][3], const double re[16],
                                          double rt, const double xp[3], const double x[3], int64_t v)
{
    double xi[3], N[8];
    inv_map_hex8(Xe, xp, xi);
    c->n_invmap++;
    double m = fmax(fabs(xi[0]), fmax(fabs(xi[1]), fabs(xi[2])));
    if (m < 1.001) {
        hex8_shape(xi, N);
        double rho = 0.0;
        for (int k = 0; k < 8; ++k) rho += N[k] * re[k];
        if (rho >= rt) {
            double dv[3] = {x[0] - xp[0], x[1] - xp[1], x[2] - xp[2]};
            write_value(c, v, norm3(dv), xp);
            return 1;
        }
    }
    return 0;
}

static int projected_on_full_segment_tet4(dist_ctx *c, const double Xe[8][3], const double re[8],
                                          double rt, const double xp[3], const double x[3], int64_t v);
static inline int projected_on_full_segment(dist_ctx *c, const double Xe[16][3], const double re[16],
                                            double rt, const double xp[3], const double x[3], int64_t v)
{
    return c->elem_type == 0 ? projected_on_full_segment_hex8(c, Xe, re, rt, xp, x, v)
                             : projected_on_full_segment_tet4(c, Xe, re, rt, xp, x, v);
}

/* barycentricCoordinates (src/SignedDistances/TriangularMeshUtils.jl:1-24) */
static void barycentric(const double x1[3], const double x2[3], const double x3[3],
                        const double n[3], const double x[3], double lam[3])
{
    double A[9] = {
        x1[1] * n[2] - x1[2] * n[1], x2[1] * n[2] - x2[2] * n[1], x3[1] * n[2] - x3[2] * n[1],
        x1[2] * n[0] - x1[0] * n[2], x2[2] * n[0] - x2[0] * n[2], x3[2] * n[0] - x3[0] * n[2],
        x1[0] * n[1] - x1[1] * n[0], x2[0] * n[1] - x2[1] * n[0], x3[0] * n[1] - x3[1] * n[0]};
    double b[3] = {x[1] * n[2] - x[2] * n[1], x[2] * n[0] - x[0] * n[2], x[0] * n[1] - x[1] * n[0]};
    int im = 0;
    double nm = fabs(n[0]);
    if (fabs(n[1]) > nm) { nm = fabs(n[1]); im = 1; }
    if (fabs(n[2]) > nm) { nm = fabs(n[2]); im = 2; }
    A[3 * im] = 1.0; A[3 * im + 1] = 1.0; A[3 * im + 2] = 1.0;
    b[im] = 1.0;
    if (lu_solve(3, A, b)) { b[0] = b[1] = b[2] = NAN; }
    lam[0] = b[0]; lam[1] = b[1]; lam[2] = b[2];
}

/* process_triangle_projection! (sdfOnDensityField.jl:628-815), HEX8 validation */
static void process_triangle(dist_ctx *c, const double Xt[3][3], int is_solid,
                             const double Xe[16][3], const double re[16], double rt)
{
    const orc_grid *g = c->g;
    double Et[3][3], n[3];
    for (int i = 0; i < 3; ++i) {
        Et[0][i] = Xt[1][i] - Xt[0][i];
        Et[1][i] = Xt[2][i] - Xt[1][i];
        Et[2][i] = Xt[0][i] - Xt[2][i];
    }
    n[0] = Et[0][1] * Et[1][2] - Et[0][2] * Et[1][1];
    n[1] = Et[0][2] * Et[1][0] - Et[0][0] * Et[1][2];
    n[2] = Et[0][0] * Et[1][1] - Et[0][1] * Et[1][0];
    double nn = norm3(n);
    n[0] /= nn; n[1] /= nn; n[2] /= nn;
    int64_t Imin[3], Imax[3];
    mini_aabb(g, Xt, 3, c->delta, Imin, Imax);
    for (int64_t I3 = Imin[2]; I3 <= Imax[2]; ++I3)
      for (int64_t I2 = Imin[1]; I2 <= Imax[1]; ++I2)
        for (int64_t I1 = Imin[0]; I1 <= Imax[0]; ++I1) {
            int64_t ii = I3 * (g->N[0] + 1) * (g->N[1] + 1) + I2 * (g->N[0] + 1) + I1;
            for (int64_t v = c->head[ii] - 1; v != -1; v = c->next[v]) {
                int64_t vi = v % (g->N[0] + 1), vj = (v / (g->N[0] + 1)) % (g->N[1] + 1);
                int64_t vk = v / ((g->N[0] + 1) * (g->N[1] + 1));
                double x[3], lam[3], xp[3], dv[3];
                grid_point(g, vi, vj, vk, x);
                c->n_tri_tests++;
                barycentric(Xt[0], Xt[1], Xt[2], n, x, lam);
                int ok = 0;
                double lmin = lam[0];
                /* Julia minimum(): NaN-propagating */
                if (lam[1] < lmin || lam[1] != lam[1]) lmin = lam[1];
                if (lam[2] < lmin || lam[2] != lam[2]) lmin = lam[2];
                if (lam[0] != lam[0]) lmin = lam[0];
                if (g_true_min) { /* every candidate: foot on the face, feet on the edges, the three vertices */
                    if (lmin >= 0.0) {
                        for (int i = 0; i < 3; ++i)
                            xp[i] = lam[0] * Xt[0][i] + lam[1] * Xt[1][i] + lam[2] * Xt[2][i];
                        for (int i = 0; i < 3; ++i) dv[i] = x[i] - xp[i];
                        double d = norm3(dv);
                        if (is_solid) write_value(c, v, d, xp);
                        else projected_on_full_segment(c, Xe, re, rt, xp, x, v);
                    }
                    for (int j = 0; j < 3; ++j) {
                        double L = norm3(Et[j]);
                        double eh[3] = {Et[j][0] / L, Et[j][1] / L, Et[j][2] / L};
                        double P = (x[0] - Xt[j][0]) * eh[0] + (x[1] - Xt[j][1]) * eh[1] +
                                   (x[2] - Xt[j][2]) * eh[2];
                        if (P >= 0 && P <= L) {
                            for (int i = 0; i < 3; ++i) xp[i] = Xt[j][i] + eh[i] * P;
                            for (int i = 0; i < 3; ++i) dv[i] = x[i] - xp[i];
                            double d = norm3(dv);
                            if (is_solid) write_value(c, v, d, xp);
                            else projected_on_full_segment(c, Xe, re, rt, xp, x, v);
                        }
                    }
                    for (int j = 0; j < 3; ++j) {
                        for (int i = 0; i < 3; ++i) { dv[i] = x[i] - Xt[j][i]; xp[i] = Xt[j][i]; }
                        double d = norm3(dv);
                        if (is_solid) write_value(c, v, d, xp);
                        else projected_on_full_segment(c, Xe, re, rt, xp, x, v);
                    }
                    continue;
                }
                if (lmin >= 0.0) {
                    for (int i = 0; i < 3; ++i)
                        xp[i] = lam[0] * Xt[0][i] + lam[1] * Xt[1][i] + lam[2] * Xt[2][i];
                    for (int i = 0; i < 3; ++i) dv[i] = x[i] - xp[i];
                    double d = norm3(dv);
                    if (is_solid) ok = write_value(c, v, d, xp);
                    else ok = projected_on_full_segment(c, Xe, re, rt, xp, x, v);
                } else {
                    for (int j = 0; j < 3; ++j) {
                        double L = norm3(Et[j]);
                        double eh[3] = {Et[j][0] / L, Et[j][1] / L, Et[j][2] / L};
                        double P = (x[0] - Xt[j][0]) * eh[0] + (x[1] - Xt[j][1]) * eh[1] +
                                   (x[2] - Xt[j][2]) * eh[2];
                        if (P >= 0 && P <= L) {
                            for (int i = 0; i < 3; ++i) xp[i] = Xt[j][i] + eh[i] * P;
                            for (int i = 0; i < 3; ++i) dv[i] = x[i] - xp[i];
                            double d = norm3(dv);
                            if (is_solid) ok = write_value(c, v, d, xp);
                            else ok = projected_on_full_segment(c, Xe, re, rt, xp, x, v);
                            if (ok) break;
                        }
                    }
                }
                if (!ok) {
                    double dd[3];
                    for (int j = 0; j < 3; ++j) {
                        for (int i = 0; i < 3; ++i) dv[i] = x[i] - Xt[j][i];
                        dd[j] = norm3(dv);
                    }
                    int idx = 0; /* findmin: first minimum, NaN wins */
                    for (int j = 1; j < 3; ++j)
                        if (dd[j] < dd[idx] || (dd[j] != dd[j] && dd[idx] == dd[idx])) idx = j;
                    for (int i = 0; i < 3; ++i) xp[i] = Xt[idx][i];
                    if (is_solid) write_value(c, v, dd[idx], xp);
                    else projected_on_full_segment(c, Xe, re, rt, xp, x, v);
                }
            }
        }
}

/* process_boundary_faces! (sdfOnDensityField.jl:489-558) */
static void process_boundary_faces(dist_ctx *c, const orc_mesh *m, int64_t el, int is_solid,
                                   const double Xe[16][3], const double re[16], double rt)
{
    for (int sg = 0; sg < m->nes; ++sg) {
        if (!face_is_boundary(m, el, sg)) continue;
        double Xs[4][3], Xc[3];
        for (int a = 0; a < m->nsn; ++a)
            for (int i = 0; i < 3; ++i) Xs[a][i] = Xe[face_node(m, sg, a)][i];
        for (int i = 0; i < 3; ++i) {
            double s = Xs[0][i];
            for (int a = 1; a < m->nsn; ++a) s += Xs[a][i];
            Xc[i] = s / (double)m->nsn;
        }
        for (int a = 0; a < m->nsn; ++a) {
            double Xt[3][3];
            int b = (a + 1) % m->nsn;
            for (int i = 0; i < 3; ++i) { Xt[0][i] = Xs[a][i]; Xt[1][i] = Xs[b][i]; Xt[2][i] = Xc[i]; }
            process_triangle(c, Xt, is_solid, Xe, re, rt);
        }
    }
}

typedef struct {
    int64_t n_solid, n_iso, n_iso_solves, n_iso_fail, n_tri_tests, n_invmap;
} orc_stats;

/* bench.py's bounded CPU sample: only grid planes with k % stride == phase are
 * evaluated (all other voxels keep the untouched values); default = every plane */
static int64_t g_kstride = 1, g_kphase = 0;
void orc_set_k_sampling(int64_t stride, int64_t phase)
{
    g_kstride = stride > 0 ? stride : 1;
    g_kphase = phase;
}

/* fill value (and zero projection points) on the sampled planes only */
static void init_sampled_planes(const orc_grid *g, double *a, double value, double *xp)
{
    const int64_t plane = (g->N[0] + 1) * (g->N[1] + 1);
    for (int64_t k = 0; k <= g->N[2]; ++k) {
        if (k % g_kstride != g_kphase) continue;
        for (int64_t v = k * plane; v < (k + 1) * plane; ++v) a[v] = value;
        if (xp) memset(xp + 3 * k * plane, 0, sizeof(double) * 3 * (size_t)plane);
    }
}

/* Test hooks around the iso-surface projections of orc_eval_distances (HEX8): a log of every (element, voxel)
 * pair in processing order, and an override that replaces the solver by a table of local coordinates in that
 * same order - tests/golden/make_slsqp_field_vectors.py feeds the field with an independent SLSQP run at the
 * reference's own tolerances and counts the voxels whose distance changes. */
static int64_t g_iso_log_cap = 0, g_iso_log_n = 0, g_iso_ovr_n = 0;
static int64_t *g_iso_log_el = NULL, *g_iso_log_v = NULL;
static double *g_iso_log_xi = NULL;
static const double *g_iso_ovr_xi = NULL;
void orc_iso_log(int64_t cap, int64_t *el, int64_t *v, double *xi /* 3*cap */)
{
    g_iso_log_cap = cap; g_iso_log_n = 0; g_iso_log_el = el; g_iso_log_v = v; g_iso_log_xi = xi;
}
int64_t orc_iso_log_count(void) { return g_iso_log_n; }
void orc_iso_override(const double *xi /* 3*n, log order; NULL = off */, int64_t n) { g_iso_ovr_xi = xi; g_iso_ovr_n = n; }

int orc_eval_distances_tet4(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_n,
                            double rho_t, const orc_grid *g, double band_factor, double *dist_out,
                            double *xp_out, orc_stats *stats);
int orc_sign_detection_tet4(const double *X, const int64_t *IEN, int64_t nel, const double *rho_n, double rho_t,
                            const orc_grid *g, double *signs);

int orc_eval_distances(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int elem_type,
                       const double *rho_n, double rho_t, const orc_grid *g, double band_factor,
                       double *dist_out, double *xp_out, orc_stats *stats)
{
    if (elem_type != 0)
        return orc_eval_distances_tet4(X, nnp, IEN, nel, rho_n, rho_t, g, band_factor, dist_out, xp_out, stats);
    orc_mesh m;
    if (mesh_init(&m, X, nnp, IEN, nel, elem_type)) return -1;
    int64_t ngp = g->ngp;
    dist_ctx c;
    memset(&c, 0, sizeof c);
    c.g = g;
    c.delta = band_factor * g->cell; /* sdfOnDensityField.jl:158 */
    /* head[] holds v + 1 (0 = empty cell) so that calloc'ed, never-touched pages read as "empty": with plane
     * sampling on a 1024^3 grid only the sampled planes' share of the work arrays is ever committed */
    c.head = (int64_t *)calloc((size_t)ngp, sizeof(int64_t));
    c.next = (int64_t *)malloc(sizeof(int64_t) * (size_t)ngp);
    c.dist = dist_out;
    c.xp = xp_out; /* may be NULL: projection points not requested */
    /* next[v] is written below for every listed point and only ever reached through head[];
     * outputs of planes that are not sampled are left untouched (callers only read the sampled planes) */
    init_sampled_planes(g, c.dist, BIG, xp_out);
    /* LinkedList (Grid.jl:47-68) */
    {
        int64_t v = 0;
        for (int64_t k = 0; k <= g->N[2]; ++k) {
          if (k % g_kstride != g_kphase) { v += (g->N[0] + 1) * (g->N[1] + 1); continue; } /* plane not sampled */
          for (int64_t j = 0; j <= g->N[1]; ++j)
            for (int64_t i = 0; i <= g->N[0]; ++i, ++v) {
                double p[3];
                grid_point(g, i, j, k, p);
                double I1 = cell_of(g, 0, p[0]), I2 = cell_of(g, 1, p[1]), I3 = cell_of(g, 2, p[2]);
                int64_t Ia = (int64_t)(I3 * (double)(g->N[0] + 1) * (double)(g->N[1] + 1) +
                                       I2 * (double)(g->N[0] + 1) + I1);
                c.next[v] = c.head[Ia] - 1;
                c.head[Ia] = v + 1;
            }
        }
    }
    int64_t n_solid = 0, n_iso = 0;
    for (int64_t el = 0; el < nel; ++el) {
        double Xe[16][3], re[16];
        double rmin = INFINITY, rmax = -INFINITY;
        for (int a = 0; a < 8; ++a) {
            int64_t n = IEN[el * 8 + a] - 1;
            for (int i = 0; i < 3; ++i) Xe[a][i] = X[3 * n + i];
            re[a] = rho_n[n];
            if (re[a] < rmin) rmin = re[a];
            if (re[a] > rmax) rmax = re[a];
        }
        if (rmin >= rho_t || rmax > rho_t) hex8_monomials(Xe, re); /* solver coefficients */
        if (rmin >= rho_t) { /* :201 */
            n_solid++;
            process_boundary_faces(&c, &m, el, 1, Xe, re, rho_t);
        } else if (rmax > rho_t) { /* :312 */
            n_iso++;
            process_boundary_faces(&c, &m, el, 0, Xe, re, rho_t); /* :584-603 */
            int64_t Imin[3], Imax[3];
            mini_aabb(g, Xe, 8, c.delta, Imin, Imax); /* :606 */
            for (int64_t I3 = Imin[2]; I3 <= Imax[2]; ++I3)
              for (int64_t I2 = Imin[1]; I2 <= Imax[1]; ++I2)
                for (int64_t I1 = Imin[0]; I1 <= Imax[0]; ++I1) {
                    int64_t ii = I3 * (g->N[0] + 1) * (g->N[1] + 1) + I2 * (g->N[0] + 1) + I1;
                    for (int64_t v = c.head[ii] - 1; v != -1; v = c.next[v]) {
                        int64_t vi = v % (g->N[0] + 1), vj = (v / (g->N[0] + 1)) % (g->N[1] + 1);
                        int64_t vk = v / ((g->N[0] + 1) * (g->N[1] + 1));
                        double x[3], xi[3], N[8], xp[3], dv[3];
                        grid_point(g, vi, vj, vk, x);
                        int it = 0;
                        if (g_iso_ovr_xi && c.n_iso_solves < g_iso_ovr_n) {
                            for (int i = 0; i < 3; ++i) xi[i] = g_iso_ovr_xi[3 * c.n_iso_solves + i];
                        } else {
                            it = iso_project_hex8(x, Xe, re, rho_t, xi); /* :616 */
                        }
                        if (g_iso_log_el) {
                            if (g_iso_log_n < g_iso_log_cap) {
                                g_iso_log_el[g_iso_log_n] = el; g_iso_log_v[g_iso_log_n] = v;
                                for (int i = 0; i < 3; ++i) g_iso_log_xi[3 * g_iso_log_n + i] = xi[i];
                            }
                            g_iso_log_n++;
                        }
                        c.n_iso_solves++;
                        if (it > ISO_MAXIT) c.n_iso_fail++;
                        hex8_shape(xi, N);
                        for (int i = 0; i < 3; ++i) {
                            double s = 0.0;
                            for (int k = 0; k < 8; ++k) s = fma(Xe[k][i], N[k], s);
                            xp[i] = s;
                            dv[i] = x[i] - s;
                        }
                        write_value(&c, v, norm3(dv), xp); /* :617-621 */
                    }
                }
        }
    }
    if (stats) {
        stats->n_solid = n_solid; stats->n_iso = n_iso;
        stats->n_iso_solves = c.n_iso_solves; stats->n_iso_fail = c.n_iso_fail;
        stats->n_tri_tests = c.n_tri_tests; stats->n_invmap = c.n_invmap;
    }
    free(c.head); free(c.next);
    mesh_free(&m);
    return 0;
}

/* ------------------------------------------------------------------ */
/* Sign_Detection_HEX8 (src/SignedDistances/SignDetection.jl:6-81)     */
/* ------------------------------------------------------------------ */
static void elem_gather_hex8(const double *X, const int64_t *IEN, const double *rho_n, int64_t el,
                             double Xe[8][3], double re[8], double mn[3], double mx[3], double *rmax)
{
    *rmax = -INFINITY;
    for (int a = 0; a < 8; ++a) {
        int64_t n = IEN[el * 8 + a] - 1;
        for (int i = 0; i < 3; ++i) {
            Xe[a][i] = X[3 * n + i];
            if (a == 0 || Xe[a][i] < mn[i]) mn[i] = Xe[a][i];
            if (a == 0 || Xe[a][i] > mx[i]) mx[i] = Xe[a][i];
        }
        re[a] = rho_n[n];
        if (re[a] > *rmax) *rmax = re[a];
    }
}

/* per-voxel state machine of SignDetection.jl:41-70 for one candidate element */
static inline void sign_visit(const double Xe[16][3], const double re[16], double rt, const double x[3],
                              double *max_local, double *sign, int *done)
{
    double xi[3], N[8];
    inv_map_hex8(Xe, x, xi);
    double m = fmax(fabs(xi[0]), fmax(fabs(xi[1]), fabs(xi[2])));
    if (g_true_min) { /* any element that holds the point decides for +1 (see write_value) */
        if (m < 1.01) {
            hex8_shape(xi, N);
            double rho = 0.0;
            for (int k = 0; k < 8; ++k) rho += N[k] * re[k];
            if (rho >= rt) { *sign = 1.0; *done = 1; }
        }
        return;
    }
    if (m < 1.01 && *max_local > m) {
        hex8_shape(xi, N);
        double rho = 0.0;
        for (int k = 0; k < 8; ++k) rho += N[k] * re[k];
        if (rho >= rt) *sign = 1.0;
        if (m < 0.95) *done = 1;
        else *max_local = m;
    }
}

/* literal O(ngp*nel) form: per voxel, ascending candidate elements (:27-70) */
int orc_sign_detection_bruteforce(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel,
                                  const double *rho_n, double rho_t, const orc_grid *g, double *signs)
{
    (void)nnp;
    double *mn = (double *)malloc(sizeof(double) * 3 * (size_t)nel);
    double *mx = (double *)malloc(sizeof(double) * 3 * (size_t)nel);
    double *rm = (double *)malloc(sizeof(double) * (size_t)nel);
    for (int64_t el = 0; el < nel; ++el) {
        double Xe[8][3], re[8];
        elem_gather_hex8(X, IEN, rho_n, el, Xe, re, mn + 3 * el, mx + 3 * el, rm + el);
    }
    int64_t v = 0;
    for (int64_t k = 0; k <= g->N[2]; ++k)
      for (int64_t j = 0; j <= g->N[1]; ++j)
        for (int64_t i = 0; i <= g->N[0]; ++i, ++v) {
            double x[3];
            grid_point(g, i, j, k, x);
            signs[v] = -1.0;
            int any = 0;
            double cmax = -INFINITY;
            for (int64_t el = 0; el < nel; ++el) {
                const double *a = mn + 3 * el, *b = mx + 3 * el;
                if (a[0] <= x[0] && a[1] <= x[1] && a[2] <= x[2] && x[0] <= b[0] && x[1] <= b[1] && x[2] <= b[2]) {
                    any = 1;
                    if (rm[el] > cmax) cmax = rm[el];
                }
            }
            if (!any || cmax < rho_t) continue; /* :36 */
            double max_local = 10.0;
            int done = 0;
            for (int64_t el = 0; el < nel && !done; ++el) {
                const double *a = mn + 3 * el, *b = mx + 3 * el;
                if (!(a[0] <= x[0] && a[1] <= x[1] && a[2] <= x[2] && x[0] <= b[0] && x[1] <= b[1] && x[2] <= b[2]))
                    continue;
                double Xe[16][3], re[16], t1[3], t2[3], t3;
                elem_gather_hex8(X, IEN, rho_n, el, Xe, re, t1, t2, &t3);
                hex8_monomials(Xe, re);
                sign_visit(Xe, re, rho_t, x, &max_local, &signs[v], &done);
            }
        }
    free(mn); free(mx); free(rm);
    return 0;
}

/* same result, element-major traversal (candidates still met in ascending
 * element order by every voxel); used for anything but tiny grids */
int orc_sign_detection(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int elem_type,
                       const double *rho_n, double rho_t, const orc_grid *g, double *signs)
{
    (void)nnp;
    if (elem_type != 0) return orc_sign_detection_tet4(X, IEN, nel, rho_n, rho_t, g, signs);
    int64_t ngp = g->ngp, nx = g->N[0] + 1, ny = g->N[1] + 1;
    double *cmax = (double *)malloc(sizeof(double) * (size_t)ngp);
    double *mloc = (double *)malloc(sizeof(double) * (size_t)ngp);
    unsigned char *flag = (unsigned char *)calloc((size_t)ngp, 1); /* bit0 any, bit1 done */
    init_sampled_planes(g, signs, -1.0, NULL);
    for (int64_t k = 0; k <= g->N[2]; ++k) { /* work arrays: only the sampled planes are ever touched */
        if (k % g_kstride != g_kphase) continue;
        for (int64_t v = k * nx * ny; v < (k + 1) * nx * ny; ++v) { cmax[v] = -INFINITY; mloc[v] = 10.0; }
    }
    for (int pass = 0; pass < 2; ++pass)
        for (int64_t el = 0; el < nel; ++el) {
            double Xe[16][3], re[16], mn[3], mx[3], rmax;
            elem_gather_hex8(X, IEN, rho_n, el, Xe, re, mn, mx, &rmax);
            if (pass == 1) hex8_monomials(Xe, re);
            int64_t lo[3], hi[3];
            for (int ax = 0; ax < 3; ++ax) { /* conservative lattice range; exact test below */
                double a = floor((mn[ax] - g->amin[ax]) / g->cell) - 1.0;
                double b = ceil((mx[ax] - g->amin[ax]) / g->cell) + 1.0;
                if (a < 0) a = 0;
                if (b > (double)g->N[ax]) b = (double)g->N[ax];
                lo[ax] = (int64_t)a; hi[ax] = (int64_t)b;
            }
            for (int64_t k = lo[2]; k <= hi[2]; ++k)
              for (int64_t j = lo[1]; j <= hi[1]; ++j)
                for (int64_t i = lo[0]; i <= hi[0]; ++i) {
                    double x[3];
                    if (k % g_kstride != g_kphase) continue;
                    grid_point(g, i, j, k, x);
                    if (!(mn[0] <= x[0] && mn[1] <= x[1] && mn[2] <= x[2] && x[0] <= mx[0] &&
                          x[1] <= mx[1] && x[2] <= mx[2]))
                        continue;
                    int64_t v = k * nx * ny + j * nx + i;
                    if (pass == 0) {
                        flag[v] |= 1;
                        if (rmax > cmax[v]) cmax[v] = rmax;
                    } else {
                        if ((flag[v] & 2) || cmax[v] < rho_t) continue;
                        int done = 0;
                        sign_visit(Xe, re, rho_t, x, &mloc[v], &signs[v], &done);
                        if (done) flag[v] |= 2;
                    }
                }
        }
    free(cmax); free(mloc); free(flag);
    return 0;
}

/* ------------------------------------------------------------------ */
/* DenseInNodes (src/MeshGrid/NodalDensities.jl:89-218)                */
/* ------------------------------------------------------------------ */
/* symmetric n x n eigen-decomposition by cyclic Jacobi (stands in for
 * LAPACK `eigen`, NodalDensities.jl:159); eigenvalues ascending, V columns */
static void jacobi_eig(int n, double *A /* n*n, destroyed */, double *w, double *V)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
        if (off == 0.0) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                double apq = A[p * n + q];
                if (apq == 0.0) continue;
                double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                double t = ((theta >= 0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < n; ++k) {
                    double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = cs * akp - sn * akq;
                    A[k * n + q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < n; ++k) {
                    double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = cs * apk - sn * aqk;
                    A[q * n + k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = cs * vkp - sn * vkq;
                    V[k * n + q] = sn * vkp + cs * vkq;
                }
            }
    }
    for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
    for (int i = 0; i < n; ++i) { /* selection sort ascending */
        int m = i;
        for (int j = i + 1; j < n; ++j)
            if (w[j] < w[m]) m = j;
        if (m != i) {
            double t = w[i]; w[i] = w[m]; w[m] = t;
            for (int k = 0; k < n; ++k) { t = V[k * n + i]; V[k * n + i] = V[k * n + m]; V[k * n + m] = t; }
        }
    }
}

int orc_dense_in_nodes(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int elem_type,
                       const double *rho_e, double *rho_n)
{
    orc_mesh m;
    if (mesh_init(&m, X, nnp, IEN, nel, elem_type)) return -1;
    int nen = m.nen;
    double *C = (double *)malloc(sizeof(double) * 3 * (size_t)nel); /* GeometricCentre :71-80 */
    for (int64_t e = 0; e < nel; ++e)
        for (int i = 0; i < 3; ++i) {
            double s = 0.0;
            for (int a = 0; a < nen; ++a) s += X[3 * (IEN[e * nen + a] - 1) + i];
            C[3 * e + i] = s / (double)nen;
        }
    for (int64_t nd = 0; nd < nnp; ++nd) {
        int64_t p0 = m.ine_ptr[nd], cnt = m.ine_ptr[nd + 1] - p0;
        const int64_t *els = m.ine + p0;
        double out = 0.0;
        if (cnt == 1) {
            out = rho_e[els[0]];                                   /* :99-100 */
        } else if (cnt > 1 && cnt < 4) {                           /* FilterForNodalDensity :117-136 */
            double L[3], Lmax = 0.0;
            for (int64_t j = 0; j < cnt; ++j) {
                double dv[3];
                for (int i = 0; i < 3; ++i) dv[i] = X[3 * nd + i] - C[3 * els[j] + i];
                L[j] = norm3(dv);
                if (L[j] > Lmax) Lmax = L[j];
            }
            Lmax = Lmax * 1.2;
            double dm = 0.0, den = 0.0;
            for (int64_t j = 0; j < cnt; ++j) {
                dm += rho_e[els[j]] * (1 - L[j] / Lmax);
                den += (1 - L[j] / Lmax);
            }
            out = dm / den;
        } else if (cnt > 3) {                                      /* NodalDensityLeastSquares :145-181 */
            double AtA[16] = {0}, Atb[4] = {0}, bsum = 0.0;
            for (int64_t j = 0; j < cnt; ++j) {
                double row[4] = {1.0, C[3 * els[j]], C[3 * els[j] + 1], C[3 * els[j] + 2]};
                for (int r = 0; r < 4; ++r) {
                    for (int c = 0; c < 4; ++c) AtA[r * 4 + c] += row[r] * row[c];
                    Atb[r] += row[r] * rho_e[els[j]];
                }
                bsum += rho_e[els[j]];
            }
            double w[4], V[16];
            jacobi_eig(4, AtA, w, V);
            /* LamReduction :190-218 */
            double wmax = w[3], wmin = w[0];
            double e1 = fabs(wmax / wmin), e2 = fabs(wmax / w[1]), e3 = fabs(wmax / w[2]);
            int first = -1; /* index of first kept eigenvalue; -1 = none */
            if (1e7 > e1 && 3e3 > e2) first = 0;
            else if (1e7 < e1 && 3e3 > e2) first = 1;
            else if (1e7 < e1 && 3e3 < e2) first = (3e3 > e3) ? 2 : 3;
            if (first < 0) {
                out = bsum / (double)cnt;
            } else {
                double b1[4], x2[4], xs[4];
                for (int c = 0; c < 4; ++c) {
                    double s = 0.0;
                    for (int r = 0; r < 4; ++r) s += V[r * 4 + c] * Atb[r];
                    b1[c] = s;
                }
                for (int c = 0; c < 4; ++c) x2[c] = (c >= first) ? b1[c] / w[c] : 0.0;
                for (int r = 0; r < 4; ++r) {
                    double s = 0.0;
                    for (int c = 0; c < 4; ++c) s += V[r * 4 + c] * x2[c];
                    xs[r] = s;
                }
                out = xs[0] + X[3 * nd] * xs[1] + X[3 * nd + 1] * xs[2] + X[3 * nd + 2] * xs[3];
            }
        }
        rho_n[nd] = out;
    }
    free(C);
    mesh_free(&m);
    return 0;
}

/* ------------------------------------------------------------------ */
/* noninteractive_sdf_grid_setup (src/MeshGrid/Grid_setup.jl:28-108)   */
/* ------------------------------------------------------------------ */
static int cmp_double(const void *a, const void *b)
{
    double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

int orc_auto_grid(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, int elem_type,
                  orc_grid *g, double *median_edge)
{
    int nen = elem_type == 0 ? 8 : 4, noe = elem_type == 0 ? 12 : 6;
    double *d = (double *)malloc(sizeof(double) * (size_t)(noe * nel));
    for (int64_t e = 0; e < nel; ++e)
        for (int k = 0; k < noe; ++k) {
            int s = elem_type == 0 ? HEX_EDGES[k][0] : TET_EDGES[k][0];
            int f = elem_type == 0 ? HEX_EDGES[k][1] : TET_EDGES[k][1];
            const double *ps = X + 3 * (IEN[e * nen + s] - 1), *pf = X + 3 * (IEN[e * nen + f] - 1);
            double dx = pf[0] - ps[0], dy = pf[1] - ps[1], dz = pf[2] - ps[2];
            d[e * noe + k] = sqrt(dx * dx + dy * dy + dz * dz);
        }
    int64_t n = noe * nel;
    qsort(d, (size_t)n, sizeof(double), cmp_double);
    double B = (n % 2) ? d[n / 2] : (d[n / 2 - 1] + d[n / 2]) / 2;
    free(d);
    double mn[3], mx[3];
    for (int i = 0; i < 3; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; }
    for (int64_t p = 0; p < nnp; ++p)
        for (int i = 0; i < 3; ++i) {
            if (X[3 * p + i] < mn[i]) mn[i] = X[3 * p + i];
            if (X[3 * p + i] > mx[i]) mx[i] = X[3 * p + i];
        }
    double ext = fmax(mx[0] - mn[0], fmax(mx[1] - mn[1], mx[2] - mn[2]));
    int64_t n_new = (int64_t)floor(ext / B); /* Grid_setup.jl:103 */
    if (median_edge) *median_edge = B;
    return orc_grid_make(mn, mx, n_new, 3, g);
}

/* ================================================================== */
/* Gauss-Legendre tables (stands in for FastGaussQuadrature 1.1.0      */
/* `gausslegendre(n)`; n = 3 uses the closed form that package returns)*/
/* ================================================================== */
void orc_gauss_legendre(int n, double *x, double *w)
{
    if (n == 3) {
        x[0] = -sqrt(3.0 / 5.0); x[1] = 0.0; x[2] = sqrt(3.0 / 5.0);
        w[0] = 5.0 / 9.0; w[1] = 8.0 / 9.0; w[2] = 5.0 / 9.0;
        return;
    }
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        double z = cos(pi * ((double)(n - 1 - i) + 0.75) / ((double)n + 0.5)); /* ascending */
        double pp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p1 = 1.0, p2 = 0.0;
            for (int j = 1; j <= n; ++j) {
                double p3 = p2;
                p2 = p1;
                p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
            }
            pp = n * (z * p1 - p2) / (z * z - 1.0);
            double dz = p1 / pp;
            z -= dz;
            if (fabs(dz) < 1e-16) break;
        }
        if ((n % 2) && i == n / 2) z = 0.0;
        /* recompute derivative at the converged node */
        {
            double p1 = 1.0, p2 = 0.0;
            for (int j = 1; j <= n; ++j) {
                double p3 = p2;
                p2 = p1;
                p1 = ((2.0 * j - 1.0) * z * p2 - (j - 1.0) * p3) / j;
            }
            pp = n * (z * p1 - p2) / (z * z - 1.0);
        }
        x[i] = z;
        w[i] = 2.0 / ((1.0 - z * z) * pp * pp);
    }
    for (int i = 0; i < n / 2; ++i) { /* enforce exact symmetry like the reference tables */
        double xa = 0.5 * (x[n - 1 - i] - x[i]), wa = 0.5 * (w[i] + w[n - 1 - i]);
        x[i] = -xa; x[n - 1 - i] = xa; w[i] = wa; w[n - 1 - i] = wa;
    }
}

static inline double det3(const double J[3][3])
{
    return J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
           J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
           J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
}

/* volume of one HEX8 restricted to {rho >= thr} by tensor Gauss quadrature
 * (MeshVolume.jl:45-72 when check == 0; Isocontour_volume.jl:54-69 otherwise) */
static double hex8_quad_volume(const double Xe[8][3], const double re[8], int n, const double *gp,
                               const double *gw, int check, double thr)
{
    double vol = 0.0;
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                double xi[3] = {gp[i], gp[j], gp[k]}, N[8], dN[8][3], J[3][3];
                hex8_shape_d(xi, N, dN);
                if (check) {
                    double v = 0.0;
                    for (int a = 0; a < 8; ++a) v += N[a] * re[a];
                    if (v < thr) continue;
                }
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) {
                        double s = 0.0;
                        for (int a = 0; a < 8; ++a) s += Xe[a][r] * dN[a][c];
                        J[r][c] = s;
                    }
                vol += gw[i] * gw[j] * gw[k] * fabs(det3(J));
            }
    return vol;
}

/* calculate_mesh_volume (src/MeshGrid/MeshVolume.jl:4-42), HEX8, single thread */
int orc_mesh_volume(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_e,
                    double *V_domain, double *V_frac)
{
    (void)nnp;
    double gp[3], gw[3], dom = 0.0, to = 0.0;
    orc_gauss_legendre(3, gp, gw);
    for (int64_t e = 0; e < nel; ++e) {
        double Xe[8][3], re[8] = {0};
        for (int a = 0; a < 8; ++a)
            for (int i = 0; i < 3; ++i) Xe[a][i] = X[3 * (IEN[e * 8 + a] - 1) + i];
        double v = hex8_quad_volume(Xe, re, 3, gp, gw, 0, 0.0);
        dom += v;
        to += v * rho_e[e];
    }
    *V_domain = dom;
    *V_frac = to / dom;
    return 0;
}

/* calculate_isocontour_volume (src/MeshGrid/Isocontour_volume.jl:1-75) */
double orc_isocontour_volume(const double *X, const int64_t *IEN, int64_t nel, const double *rho_n,
                             double thr)
{
    double g15[15], w15[15], g3[3], w3[3], total = 0.0;
    orc_gauss_legendre(15, g15, w15);
    orc_gauss_legendre(3, g3, w3);
    for (int64_t e = 0; e < nel; ++e) {
        double Xe[8][3], re[8], mn = INFINITY, mx = -INFINITY;
        for (int a = 0; a < 8; ++a) {
            int64_t n = IEN[e * 8 + a] - 1;
            for (int i = 0; i < 3; ++i) Xe[a][i] = X[3 * n + i];
            re[a] = rho_n[n];
            if (re[a] < mn) mn = re[a];
            if (re[a] > mx) mx = re[a];
        }
        if (mx < thr) continue;
        if (mn >= thr) total += hex8_quad_volume(Xe, re, 3, g3, w3, 0, thr);
        else total += hex8_quad_volume(Xe, re, 15, g15, w15, 1, thr);
    }
    return total;
}

/* find_threshold_for_volume (Isocontour_volume.jl:77-154); returns -1 if out of range (:93-95) */
int orc_find_threshold(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_n,
                       double target_volume, double tol, int maxit, double *rho_t, int *iters)
{
    (void)nnp;
    double lo = 0.0, hi = 1.0;
    double vmin = orc_isocontour_volume(X, IEN, nel, rho_n, hi);
    double vmax = orc_isocontour_volume(X, IEN, nel, rho_n, lo);
    if (target_volume > vmax || target_volume < vmin) return -1;
    int it = 0;
    double best = 0.0, best_err = INFINITY;
    while (it < maxit) {
        double thr = (lo + hi) / 2;
        double v = orc_isocontour_volume(X, IEN, nel, rho_n, thr);
        double err = fabs(v - target_volume) / target_volume;
        if (err < best_err) { best = thr; best_err = err; }
        if (err < tol) break;
        if (v > target_volume) lo = thr; else hi = thr;
        it++;
    }
    *rho_t = best;
    if (iters) *iters = it;
    return 0;
}

/* TET4 iso-volume.  The reference has none (calculate_isocontour_volume hard-codes 8 nodes,
 * Isocontour_volume.jl:27-38); SURVEY 8(f)2 asks for one.  Assembled from the reference's own pieces: the
 * classification of Isocontour_volume.jl:40-52 (skip / whole / cut) with the collapsed-cube rule of
 * MeshVolume.jl:75-117 (3^3 points for whole elements, 15^3 with the point test of :62-64 for cut ones; the same
 * `jacobian_transform`), so that volume(0) equals calculate_mesh_volume's V_domain for TET4. */
static double tet4_quad_volume(const double xe[4][3], const double re[4], int n, const double *gp, const double *gw,
                               int check, double thr)
{
    double J[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int a = 0; a < 4; ++a) {
                double dn = (a == c) ? 1.0 : ((a == 3) ? -1.0 : 0.0);
                s += xe[a][r] * dn;
            }
            J[r][c] = s;
        }
    double adet = fabs(det3(J)), vol = 0.0;
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                double xi = (gp[i] + 1.0) / 2.0;
                double eta = (gp[j] + 1.0) / 2.0 * (1.0 - xi);
                double zeta = (gp[k] + 1.0) / 2.0 * (1.0 - xi - eta);
                if (xi < 0 || eta < 0 || zeta < 0 || xi + eta + zeta > 1.0) continue;
                if (check) {
                    double v = xi * re[0] + eta * re[1] + zeta * re[2] + (1.0 - xi - eta - zeta) * re[3];
                    if (v < thr) continue;
                }
                double jt = (1.0 - xi) * (1.0 - xi) * (1.0 - xi - eta) / 8.0;
                vol += gw[i] * gw[j] * gw[k] * adet * jt;
            }
    return vol;
}

double orc_isocontour_volume_tet4(const double *X, const int64_t *IEN, int64_t nel, const double *rho_n, double thr)
{
    double g15[15], w15[15], g3[3], w3[3], total = 0.0;
    orc_gauss_legendre(15, g15, w15);
    orc_gauss_legendre(3, g3, w3);
    for (int64_t e = 0; e < nel; ++e) {
        double xe[4][3], re[4], mn = INFINITY, mx = -INFINITY;
        for (int a = 0; a < 4; ++a) {
            int64_t n = IEN[e * 4 + a] - 1;
            for (int i = 0; i < 3; ++i) xe[a][i] = X[3 * n + i];
            re[a] = rho_n[n];
            if (re[a] < mn) mn = re[a];
            if (re[a] > mx) mx = re[a];
        }
        if (mx < thr) continue;
        if (mn >= thr) total += tet4_quad_volume(xe, re, 3, g3, w3, 0, thr);
        else total += tet4_quad_volume(xe, re, 15, g15, w15, 1, thr);
    }
    return total;
}

/* the bisection of find_threshold_for_volume (Isocontour_volume.jl:77-154) over the TET4 iso-volume */
int orc_find_threshold_tet4(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_n,
                            double target_volume, double tol, int maxit, double *rho_t, int *iters)
{
    (void)nnp;
    double lo = 0.0, hi = 1.0;
    double vmin = orc_isocontour_volume_tet4(X, IEN, nel, rho_n, hi);
    double vmax = orc_isocontour_volume_tet4(X, IEN, nel, rho_n, lo);
    if (target_volume > vmax || target_volume < vmin) return -1;
    int it = 0;
    double best = 0.0, best_err = INFINITY;
    while (it < maxit) {
        double thr = (lo + hi) / 2;
        double v = orc_isocontour_volume_tet4(X, IEN, nel, rho_n, thr);
        double err = fabs(v - target_volume) / target_volume;
        if (err < best_err) { best = thr; best_err = err; }
        if (err < tol) break;
        if (v > target_volume) lo = thr; else hi = thr;
        it++;
    }
    *rho_t = best;
    if (iters) *iters = it;
    return 0;
}

/* ================================================================== */
/* remove_sdf_artifacts! (src/SignedDistances/SdfArtifactRemoval.jl:134-245) */
/* serial union-find semantics (analyze_sdf_components :271-285)       */
/* ================================================================== */
static int64_t uf_find(int64_t *p, int64_t x)
{
    int64_t r = x;
    while (p[r] != r) r = p[r];
    while (p[x] != r) { int64_t n = p[x]; p[x] = r; x = n; }
    return r;
}

int64_t orc_remove_artifacts(double *sdf, const orc_grid *g, double threshold, double min_ratio)
{
    int64_t ngp = g->ngp, nx = g->N[0] + 1, ny = g->N[1] + 1, nz = g->N[2] + 1;
    int64_t *par = (int64_t *)malloc(sizeof(int64_t) * (size_t)ngp);
    int64_t *sz = (int64_t *)calloc((size_t)ngp, sizeof(int64_t));
    int64_t interior = 0;
    for (int64_t v = 0; v < ngp; ++v) { par[v] = v; interior += (sdf[v] >= threshold); }
    if (interior == 0) { free(par); free(sz); return 0; }
    for (int64_t k = 0; k < nz; ++k)
        for (int64_t j = 0; j < ny; ++j)
            for (int64_t i = 0; i < nx; ++i) {
                int64_t v = (k * ny + j) * nx + i;
                if (!(sdf[v] >= threshold)) continue;
                int64_t nb[3] = {i + 1 < nx ? v + 1 : -1, j + 1 < ny ? v + nx : -1, k + 1 < nz ? v + nx * ny : -1};
                for (int q = 0; q < 3; ++q)
                    if (nb[q] >= 0 && sdf[nb[q]] >= threshold) {
                        int64_t a = uf_find(par, v), b = uf_find(par, nb[q]);
                        if (a != b) par[b > a ? b : a] = (b > a ? a : b);
                    }
            }
    int64_t largest = 0, largest_root = -1;
    for (int64_t v = 0; v < ngp; ++v)
        if (sdf[v] >= threshold) sz[uf_find(par, v)]++;
    for (int64_t v = 0; v < ngp; ++v)
        if (sz[v] > largest) { largest = sz[v]; largest_root = v; }
    double t = min_ratio * (double)largest;
    int64_t min_size = (int64_t)nearbyint(t); /* Julia round(Int, x): ties to even (:206) */
    if (min_size < 1) min_size = 1;
    int64_t flipped = 0;
    for (int64_t v = 0; v < ngp; ++v)
        if (sdf[v] >= threshold) {
            int64_t r = uf_find(par, v);
            if (r != largest_root && sz[r] < min_size) { sdf[v] = -fabs(sdf[v]); flipped++; }
        }
    free(par); free(sz);
    return flipped;
}

/* ================================================================== */
/* calculate_volume_from_sdf (src/SdfSmoothing/CalcVolumeFromSDF.jl:26-125) */
/* Float32 throughout; single thread = sequential k,j,i accumulation    */
/* ================================================================== */
float orc_volume_from_sdf(const float *sdf, int64_t nx, int64_t ny, int64_t nz, float edge, float iso,
                          int order)
{
    double gpd[64], gwd[64];
    float gp[64], gw[64];
    orc_gauss_legendre(order, gpd, gwd);
    for (int i = 0; i < order; ++i) { gp[i] = (float)gpd[i]; gw[i] = (float)gwd[i]; }
    const float elvol = edge * edge * edge;
    const float jac = elvol / 8.0f;
    float total = 0.0f;
#define S(i, j, k) sdf[((k) * ny + (j)) * nx + (i)]
    for (int64_t k = 0; k < nz - 1; ++k)
        for (int64_t j = 0; j < ny - 1; ++j)
            for (int64_t i = 0; i < nx - 1; ++i) {
                float c000 = S(i, j, k), c100 = S(i + 1, j, k), c010 = S(i, j + 1, k), c110 = S(i + 1, j + 1, k);
                float c001 = S(i, j, k + 1), c101 = S(i + 1, j, k + 1), c011 = S(i, j + 1, k + 1),
                      c111 = S(i + 1, j + 1, k + 1);
                float mn = fminf(fminf(fminf(c000, c100), fminf(c010, c110)), fminf(fminf(c001, c101), fminf(c011, c111)));
                float mx = fmaxf(fmaxf(fmaxf(c000, c100), fmaxf(c010, c110)), fmaxf(fmaxf(c001, c101), fmaxf(c011, c111)));
                if (mx < iso) continue;
                if (mn >= iso) { total += elvol; continue; }
                float part = 0.0f;
                for (int kq = 0; kq < order; ++kq) {
                    float zeta = (gp[kq] + 1) / 2;
                    for (int jq = 0; jq < order; ++jq) {
                        float eta = (gp[jq] + 1) / 2;
                        for (int iq = 0; iq < order; ++iq) {
                            float xi = (gp[iq] + 1) / 2;
                            float c00 = c000 * (1.0f - xi) + c100 * xi;
                            float c01 = c001 * (1.0f - xi) + c101 * xi;
                            float c10 = c010 * (1.0f - xi) + c110 * xi;
                            float c11 = c011 * (1.0f - xi) + c111 * xi;
                            float c0 = c00 * (1.0f - eta) + c10 * eta;
                            float c1 = c01 * (1.0f - eta) + c11 * eta;
                            float p = c0 * (1.0f - zeta) + c1 * zeta;
                            if (p >= iso) part += gw[iq] * gw[jq] * gw[kq] * jac;
                        }
                    }
                }
                total += part;
            }
#undef S
    return total;
}

/* ================================================================== */
/* RBFs_smoothing (src/SdfSmoothing/RBFs4Smoothing.jl:321-377)         */
/* Float32 values, Float64 sigma inside exp, as in the reference.      */
/* KDTree/knn (NearestNeighbors 0.4.22) on a regular lattice = fixed   */
/* stencil: neighbours are visited by increasing lattice distance      */
/* (ties: dz,dy,dx) - the reference's tie order is unspecified (A16).  */
/* ================================================================== */
/* process_vector (:15-22); returns -1 if every value is a sentinel (A15) */
int orc_process_vector(const double *v, int64_t n, float *out)
{
    float mx = -1.0f;
    for (int64_t i = 0; i < n; ++i) {
        float f = (float)v[i];
        out[i] = f;
        if (fabsf(f) < 1.0e9f && fabsf(f) > mx) mx = fabsf(f);
    }
    if (mx < 0.0f) return -1;
    const float rtol = 3.4526698e-4f; /* sqrt(eps(Float32)) */
    for (int64_t i = 0; i < n; ++i) {
        float a = fabsf(out[i]);
        float big = a > 1.0e10f ? a : 1.0e10f;
        if (fabsf(a - 1.0e10f) <= rtol * big) out[i] = (out[i] > 0 ? 1.0f : (out[i] < 0 ? -1.0f : 0.0f)) * mx;
    }
    return 0;
}

typedef struct {
    int n;
    int off[512][3]; /* coarse offsets (dx,dy,dz) relative to the base coarse index */
} rbf_stencil;

#define RBF_KNN 124 /* knn(kdtree, p, 124, true) (:238): the 124 nearest in-bounds nodes at most */

/* neighbours of a target point with sub-index frac (0..s-1 per axis) in a lattice refined s times: lattice
 * distance^2 (in 1/s cells) up to 5 % beyond the support radius R = sqrt(R2) cells, from offsets within
 * ceil(R') + 1 cells on both sides; returns -1 when they do not fit */
static int rbf_build_stencil(int s, const int frac[3], rbf_stencil *st, double R2)
{
    const int d2max = (int)floor(R2 * 1.05 * s * s + 0.25);
    const int B = (int)ceil(sqrt(R2 * 1.05)) + 1;
    int (*cand)[4] = (int (*)[4])malloc(sizeof(int[4]) * (size_t)(2 * B + 1) * (2 * B + 1) * (2 * B + 1));
    int n = 0;
    for (int dz = -B; dz <= B; ++dz)
        for (int dy = -B; dy <= B; ++dy)
            for (int dx = -B; dx <= B; ++dx) {
                int ex = dx * s - frac[0], ey = dy * s - frac[1], ez = dz * s - frac[2];
                int d2 = ex * ex + ey * ey + ez * ez;
                if (d2 > d2max) continue;
                cand[n][0] = d2; cand[n][1] = dz; cand[n][2] = dy; cand[n][3] = dx;
                n++;
            }
    if (n > 512) { free(cand); return -1; }
    for (int i = 1; i < n; ++i) { /* insertion sort by (d2, dz, dy, dx) */
        int t[4] = {cand[i][0], cand[i][1], cand[i][2], cand[i][3]}, j = i - 1;
        while (j >= 0 && (cand[j][0] > t[0] || (cand[j][0] == t[0] && (cand[j][1] > t[1] ||
               (cand[j][1] == t[1] && (cand[j][2] > t[2] || (cand[j][2] == t[2] && cand[j][3] > t[3]))))))) {
            for (int q = 0; q < 4; ++q) cand[j + 1][q] = cand[j][q];
            j--;
        }
        for (int q = 0; q < 4; ++q) cand[j + 1][q] = t[q];
    }
    st->n = n;
    for (int i = 0; i < n; ++i) { st->off[i][0] = cand[i][3]; st->off[i][1] = cand[i][2]; st->off[i][2] = cand[i][1]; }
    free(cand);
    return 0;
}

/* create_grid (:36-46): Float32 `range(min, max, length)` */
static void rbf_coarse_coords(double mn, double mx, int64_t n, float *c)
{
    double a = (double)(float)mn, b = (double)(float)mx;
    for (int64_t i = 0; i < n; ++i) c[i] = (float)(a + (double)i * (b - a) / (double)(n - 1));
    c[n - 1] = (float)mx;
}

typedef struct {
    int64_t nx, ny, nz;
    float *cx, *cy, *cz;
    double sigma;
    float max_distance;
    double thr;
    int tap_r; /* matrix rows reach this many cells per axis */
} rbf_ctx;

/* rbf_interpolation_kdtree (:219-248): targets tx/ty/tz, refined s times w.r.t. the coarse lattice */
static int rbf_apply(const rbf_ctx *c, const float *w, int s, int64_t tnx, int64_t tny, int64_t tnz,
                     const float *tx, const float *ty, const float *tz, float *out)
{
    rbf_stencil *st = (rbf_stencil *)malloc(sizeof(rbf_stencil) * (size_t)(s * s * s));
    for (int fz = 0; fz < s; ++fz)
        for (int fy = 0; fy < s; ++fy)
            for (int fx = 0; fx < s; ++fx) {
                int fr[3] = {fx, fy, fz};
                if (rbf_build_stencil(s, fr, &st[(fz * s + fy) * s + fx], -log(c->thr))) { free(st); return -1; }
            }
    for (int64_t k = 0; k < tnz; ++k)
        for (int64_t j = 0; j < tny; ++j)
            for (int64_t i = 0; i < tnx; ++i) {
                const rbf_stencil *S = &st[((k % s) * s + (j % s)) * s + (i % s)];
                int64_t bi = i / s, bj = j / s, bk = k / s;
                float acc = 0.0f;
                int seen = 0;
                for (int q = 0; q < S->n; ++q) {
                    int64_t ci = bi + S->off[q][0], cj = bj + S->off[q][1], ck = bk + S->off[q][2];
                    if (ci < 0 || cj < 0 || ck < 0 || ci >= c->nx || cj >= c->ny || ck >= c->nz) continue;
                    if (++seen > RBF_KNN) break;
                    float dx = tx[i] - c->cx[ci], dy = ty[j] - c->cy[cj], dz = tz[k] - c->cz[ck];
                    float dist = sqrtf(dx * dx + dy * dy + dz * dz);
                    if (dist <= c->max_distance) {
                        double t = (double)dist / c->sigma;
                        acc = (float)((double)acc + (double)w[(ck * c->ny + cj) * c->nx + ci] * exp(-(t * t)));
                    }
                }
                out[(k * tny + j) * tnx + i] = acc;
            }
    free(st);
    return 0;
}

/* y = K x with K from compute_sparse_kernel_matrix (:142-176): Float32 entries
 * Float32(exp(-(r/sigma)^2)) kept if > threshold; SparseMatrixCSC * vector accumulates each
 * row in ascending column (= linear index) order, in Float32 */
static void rbf_matvec(const rbf_ctx *c, const float *x, float *y)
{
    for (int64_t k = 0; k < c->nz; ++k)
        for (int64_t j = 0; j < c->ny; ++j)
            for (int64_t i = 0; i < c->nx; ++i) {
                float acc = 0.0f;
                for (int64_t ck = k - c->tap_r; ck <= k + c->tap_r; ++ck)
                    for (int64_t cj = j - c->tap_r; cj <= j + c->tap_r; ++cj)
                        for (int64_t ci = i - c->tap_r; ci <= i + c->tap_r; ++ci) {
                            if (ci < 0 || cj < 0 || ck < 0 || ci >= c->nx || cj >= c->ny || ck >= c->nz) continue;
                            float dx = c->cx[i] - c->cx[ci], dy = c->cy[j] - c->cy[cj], dz = c->cz[k] - c->cz[ck];
                            float r = sqrtf(dx * dx + dy * dy + dz * dz);
                            double t = (double)r / c->sigma;
                            double val = exp(-(t * t));
                            if (val > c->thr) acc += (float)val * x[(ck * c->ny + cj) * c->nx + ci];
                        }
                y[(k * c->ny + j) * c->nx + i] = acc;
            }
}

static float f32_dot(const float *a, const float *b, int64_t n)
{
    double s = 0.0; /* BLAS sdot/snrm2 stand-in: double accumulation, Float32 result */
    for (int64_t i = 0; i < n; ++i) s += (double)a[i] * (double)b[i];
    return (float)s;
}

/* IterativeSolvers.cg defaults (0.9.4): x0 = 0, reltol = sqrt(eps(Float32)), maxiter = n */
static int rbf_cg(const rbf_ctx *c, const float *b, float *x, int64_t n)
{
    float *r = (float *)malloc(sizeof(float) * (size_t)n), *u = (float *)calloc((size_t)n, sizeof(float));
    float *q = (float *)malloc(sizeof(float) * (size_t)n);
    memcpy(r, b, sizeof(float) * (size_t)n);
    memset(x, 0, sizeof(float) * (size_t)n);
    float residual = sqrtf(f32_dot(r, r, n)), prev = 1.0f;
    const float tol = 3.4526698e-4f * residual;
    int it = 0;
    while (!(residual <= tol) && it < n) {
        float beta = (residual * residual) / (prev * prev);
        for (int64_t i = 0; i < n; ++i) u[i] = r[i] + beta * u[i];
        rbf_matvec(c, u, q);
        float alpha = (residual * residual) / f32_dot(u, q, n);
        for (int64_t i = 0; i < n; ++i) { x[i] += alpha * u[i]; r[i] -= alpha * q[i]; }
        prev = residual;
        residual = sqrtf(f32_dot(r, r, n));
        it++;
    }
    free(r); free(u); free(q);
    return it;
}

/* LS_Threshold (:265-300) */
static float rbf_ls_threshold(const float *lsf, int64_t nx, int64_t ny, int64_t nz, float edge,
                              double target_volume, int *iters)
{
    int64_t n = nx * ny * nz;
    float lo = lsf[0], hi = lsf[0];
    for (int64_t i = 1; i < n; ++i) { if (lsf[i] < lo) lo = lsf[i]; if (lsf[i] > hi) hi = lsf[i]; }
    float *sh = (float *)malloc(sizeof(float) * (size_t)n);
    double eps = 1.0;
    float th = 0.0f;
    int it = 0;
    while (it < 40 && eps > 1.0e-4) {
        th = (lo + hi) / 2;
        for (int64_t i = 0; i < n; ++i) sh[i] = lsf[i] - th;
        float vol = orc_volume_from_sdf(sh, nx, ny, nz, edge, 0.0f, 9);
        eps = fabs(target_volume - (double)vol);
        if ((double)vol > target_volume) lo = th; else hi = th;
        it++;
    }
    free(sh);
    if (iters) *iters = it;
    return -th;
}

/* RBFs_smoothing (:321-377). fine_out has prod(N*smooth+1) entries. */
int orc_rbf_smoothing(const double *sdf, const orc_grid *g, int is_interp, int smooth, double kthr,
                      double target_volume, float *fine_out, float *th_out, int *cg_iters, float *lsf_out)
{
    rbf_ctx c;
    c.nx = g->N[0] + 1; c.ny = g->N[1] + 1; c.nz = g->N[2] + 1;
    int64_t n = c.nx * c.ny * c.nz;
    float *dm = (float *)malloc(sizeof(float) * (size_t)n);
    if (orc_process_vector(sdf, n, dm)) { free(dm); return -1; }
    c.cx = (float *)malloc(sizeof(float) * (size_t)c.nx);
    c.cy = (float *)malloc(sizeof(float) * (size_t)c.ny);
    c.cz = (float *)malloc(sizeof(float) * (size_t)c.nz);
    rbf_coarse_coords(g->amin[0], g->amax[0], c.nx, c.cx);
    rbf_coarse_coords(g->amin[1], g->amax[1], c.ny, c.cy);
    rbf_coarse_coords(g->amin[2], g->amax[2], c.nz, c.cz);
    c.sigma = g->cell;                                        /* :346 */
    c.thr = kthr;
    c.max_distance = (float)sqrt(-log(kthr) * c.sigma * c.sigma); /* :221 */
    c.tap_r = (int)floor(sqrt(-log(kthr) * 1.05 + 0.25)); /* support radius + 5 %: nothing beyond passes `> thr` */
    float *w = (float *)malloc(sizeof(float) * (size_t)n);
    int its = 0;
    if (is_interp) its = rbf_cg(&c, dm, w, n);                /* :351-352 */
    else memcpy(w, dm, sizeof(float) * (size_t)n);            /* :353 */
    if (cg_iters) *cg_iters = its;
    float *lsf = (float *)malloc(sizeof(float) * (size_t)n);
    if (rbf_apply(&c, w, 1, c.nx, c.ny, c.nz, c.cx, c.cy, c.cz, lsf)) { /* :357 */
        free(dm); free(w); free(lsf); free(c.cx); free(c.cy); free(c.cz);
        return -2;
    }
    if (lsf_out) memcpy(lsf_out, lsf, sizeof(float) * (size_t)n);
    /* calculate_volume_from_sdf takes the edge from the coarse grid (CalcVolumeFromSDF.jl:38-40) */
    float ex = c.cx[1] - c.cx[0], ey = 0.0f, ez = 0.0f;
    float edge = sqrtf(ex * ex + ey * ey + ez * ez);
    float th = rbf_ls_threshold(lsf, c.nx, c.ny, c.nz, edge, target_volume, NULL); /* :359 */
    if (th_out) *th_out = th;
    /* fine grid (:60-74): uniform step dx from the x axis, explicit Float32 arithmetic */
    int64_t fx = g->N[0] * smooth + 1, fy = g->N[1] * smooth + 1, fz = g->N[2] * smooth + 1;
    float xmin = (float)g->amin[0], xmax = (float)g->amax[0], ymin = (float)g->amin[1], zmin = (float)g->amin[2];
    float dx = (xmax - xmin) / (float)(fx - 1);
    float *tx = (float *)malloc(sizeof(float) * (size_t)fx), *ty = (float *)malloc(sizeof(float) * (size_t)fy);
    float *tz = (float *)malloc(sizeof(float) * (size_t)fz);
    for (int64_t i = 0; i < fx; ++i) tx[i] = xmin + (float)i * dx;
    for (int64_t i = 0; i < fy; ++i) ty[i] = ymin + (float)i * dx;
    for (int64_t i = 0; i < fz; ++i) tz[i] = zmin + (float)i * dx;
    if (rbf_apply(&c, w, smooth, fx, fy, fz, tx, ty, tz, fine_out)) { /* :363 */
        free(dm); free(w); free(lsf); free(tx); free(ty); free(tz); free(c.cx); free(c.cy); free(c.cz);
        return -2;
    }
    for (int64_t i = 0; i < fx * fy * fz; ++i) fine_out[i] = fine_out[i] + th; /* :366 */
    free(dm); free(w); free(lsf); free(tx); free(ty); free(tz); free(c.cx); free(c.cy); free(c.cz);
    return 0;
}

/* ================================================================== */
/* TET4                                                                */
/* ================================================================== */
/* shape_functions(TET4, lambda) (ShapeFunctions.jl:18-28): N = [l1,l2,l3, 1 - sum(l)] */
static inline void tet4_shape(const double l[3], double N[4])
{
    N[0] = l[0]; N[1] = l[1]; N[2] = l[2];
    N[3] = 1.0 - ((l[0] + l[1]) + l[2]);
}

/* find_local_coordinates, TET4 (FindLocalCoordinates.jl:110-149): 3x3 solve for (l2,l3,l4),
 * l1 = 1 - sum; valid <=> all four >= 0 and their left-to-right sum <= 1.0 (ElementTypes.jl:104-106);
 * returns [l1,l2,l3] or (10,10,10) */
static int find_local_tet4(const double Xe[8][3], const double x[3], double loc[3])
{
    double A[9], b[3];
    for (int i = 0; i < 3; ++i) {
        A[3 * i + 0] = Xe[1][i] - Xe[0][i];
        A[3 * i + 1] = Xe[2][i] - Xe[0][i];
        A[3 * i + 2] = Xe[3][i] - Xe[0][i];
        b[i] = x[i] - Xe[0][i];
    }
    if (lu_solve(3, A, b)) { loc[0] = loc[1] = loc[2] = 10.0; return 0; }
    double l1 = 1.0 - ((b[0] + b[1]) + b[2]);
    double l[4] = {l1, b[0], b[1], b[2]};
    int ok = l[0] >= 0.0 && l[1] >= 0.0 && l[2] >= 0.0 && l[3] >= 0.0 && (((l[0] + l[1]) + l[2]) + l[3]) <= 1.0;
    if (!ok) { loc[0] = loc[1] = loc[2] = 10.0; return 0; }
    loc[0] = l1; loc[1] = b[0]; loc[2] = b[1];
    return 1;
}

/* IsProjectedOnFullSegment, TET4 branch (sdfOnDensityField.jl:92-113) */
static int projected_on_full_segment_tet4(dist_ctx *c, const double Xe[8][3], const double re[8],
                                          double rt, const double xp[3], const double x[3], int64_t v)
{
    double loc[3], N[4];
    find_local_tet4(Xe, xp, loc);
    c->n_invmap++;
    double sum = (loc[0] + loc[1]) + loc[2];
    int valid = loc[0] >= 0.0 && loc[1] >= 0.0 && loc[2] >= 0.0 && sum <= 1.0 && sum <= 1.001; /* :98 */
    if (valid) {
        tet4_shape(loc, N);
        double rho = 0.0;
        for (int k = 0; k < 4; ++k) rho += N[k] * re[k];
        if (rho >= rt) {
            double dv[3] = {x[0] - xp[0], x[1] - xp[1], x[2] - xp[2]};
            write_value(c, v, norm3(dv), xp);
            return 1;
        }
    }
    return 0;
}

/* compute_coords_on_iso, TET4 (ComputeCoordsOnIso.jl:90-181): closest point of the planar polygon
 * {p in tet : rho(p) = rho_t} (affine map, linear density => convex QP with a unique minimiser; the
 * reference solves it with SLSQP from the centroid).  Solved in closed form: project x onto the
 * iso-plane; if the foot lies in the tetrahedron that is the answer, otherwise the nearest point of
 * the polygon's edges (one segment per tetrahedron face crossed by the plane).  Returns natural
 * coordinates (l1,l2,l3). */
static void iso_project_tet4(const double x[3], const double Xe[8][3], const double re[8], double rt,
                             double lam[3])
{
    double A[3][3], Ai[3][3];
    for (int i = 0; i < 3; ++i) { A[i][0] = Xe[1][i] - Xe[0][i]; A[i][1] = Xe[2][i] - Xe[0][i]; A[i][2] = Xe[3][i] - Xe[0][i]; }
    double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    double c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
    Ai[0][0] = c00 / det; Ai[1][0] = c01 / det; Ai[2][0] = c02 / det;
    Ai[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
    Ai[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
    Ai[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
    Ai[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
    Ai[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
    Ai[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    double dr[3] = {re[1] - re[0], re[2] - re[0], re[3] - re[0]}, gr[3];
    for (int i = 0; i < 3; ++i) gr[i] = Ai[0][i] * dr[0] + Ai[1][i] * dr[1] + Ai[2][i] * dr[2]; /* physical gradient */
    double g2 = gr[0] * gr[0] + gr[1] * gr[1] + gr[2] * gr[2];
    double d0[3] = {x[0] - Xe[0][0], x[1] - Xe[0][1], x[2] - Xe[0][2]};
    double rho_x = re[0] + (gr[0] * d0[0] + gr[1] * d0[1] + gr[2] * d0[2]);
    double tq = (rho_x - rt) / g2;
    double best[3] = {0, 0, 0}, bestd = INFINITY;
    {
        double q[3] = {x[0] - tq * gr[0], x[1] - tq * gr[1], x[2] - tq * gr[2]};
        double dq[3] = {q[0] - Xe[0][0], q[1] - Xe[0][1], q[2] - Xe[0][2]}, l[4];
        for (int i = 0; i < 3; ++i) l[i + 1] = Ai[i][0] * dq[0] + Ai[i][1] * dq[1] + Ai[i][2] * dq[2];
        l[0] = 1.0 - ((l[1] + l[2]) + l[3]);
        if (l[0] >= 0.0 && l[1] >= 0.0 && l[2] >= 0.0 && l[3] >= 0.0) {
            best[0] = q[0]; best[1] = q[1]; best[2] = q[2];
            bestd = 0.0; /* the foot of the perpendicular: nothing on the polygon is closer */
        }
    }
    if (bestd != 0.0) {
        for (int f = 0; f < 4; ++f) {
            const int *fn = TET_ISN[f];
            double P[3][3];
            int np = 0;
            for (int e = 0; e < 3; ++e) {
                int a = fn[e], b = fn[(e + 1) % 3];
                double ra = re[a] - rt, rb = re[b] - rt;
                if (ra * rb <= 0.0 && re[a] != re[b]) {
                    double t = (rt - re[a]) / (re[b] - re[a]);
                    for (int i = 0; i < 3; ++i) P[np][i] = Xe[a][i] + t * (Xe[b][i] - Xe[a][i]);
                    np++;
                }
            }
            if (np < 2) continue;
            /* segment between the two crossings that are farthest apart (np == 3 only if it grazes a vertex) */
            int ia = 0, ib = 1;
            if (np == 3) {
                double d01 = 0, d02 = 0, d12 = 0;
                for (int i = 0; i < 3; ++i) {
                    d01 += (P[0][i] - P[1][i]) * (P[0][i] - P[1][i]);
                    d02 += (P[0][i] - P[2][i]) * (P[0][i] - P[2][i]);
                    d12 += (P[1][i] - P[2][i]) * (P[1][i] - P[2][i]);
                }
                if (d02 >= d01 && d02 >= d12) { ia = 0; ib = 2; }
                else if (d12 >= d01 && d12 >= d02) { ia = 1; ib = 2; }
            }
            double ab[3], ax[3], ab2 = 0.0, dot = 0.0;
            for (int i = 0; i < 3; ++i) { ab[i] = P[ib][i] - P[ia][i]; ax[i] = x[i] - P[ia][i]; ab2 += ab[i] * ab[i]; dot += ax[i] * ab[i]; }
            double s = ab2 > 0.0 ? dot / ab2 : 0.0;
            s = fmin(fmax(s, 0.0), 1.0);
            double p[3], dd = 0.0;
            for (int i = 0; i < 3; ++i) { p[i] = P[ia][i] + s * ab[i]; dd += (x[i] - p[i]) * (x[i] - p[i]); }
            if (dd < bestd) { bestd = dd; best[0] = p[0]; best[1] = p[1]; best[2] = p[2]; }
        }
    }
    if (bestd == INFINITY) { lam[0] = lam[1] = lam[2] = 0.25; return; } /* no polygon: the SLSQP start */
    double db[3] = {best[0] - Xe[0][0], best[1] - Xe[0][1], best[2] - Xe[0][2]}, l234[3];
    for (int i = 0; i < 3; ++i) l234[i] = Ai[i][0] * db[0] + Ai[i][1] * db[1] + Ai[i][2] * db[2];
    lam[0] = 1.0 - ((l234[0] + l234[1]) + l234[2]);
    lam[1] = l234[0];
    lam[2] = l234[1];
}

int orc_iso_project_tet4(const double x[3], const double *Xe4 /* 4*3 */, const double re4[4], double rt, double lam[3])
{
    double Xe[8][3] = {{0}}, re[8] = {0};
    for (int a = 0; a < 4; ++a) { for (int i = 0; i < 3; ++i) Xe[a][i] = Xe4[3 * a + i]; re[a] = re4[a]; }
    iso_project_tet4(x, Xe, re, rt, lam);
    return 0;
}

int orc_eval_distances_tet4(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_n,
                            double rho_t, const orc_grid *g, double band_factor, double *dist_out,
                            double *xp_out, orc_stats *stats)
{
    orc_mesh m;
    if (mesh_init(&m, X, nnp, IEN, nel, 1)) return -1;
    int64_t ngp = g->ngp;
    dist_ctx c;
    memset(&c, 0, sizeof c);
    c.g = g;
    c.elem_type = 1;
    c.delta = band_factor * g->cell;
    c.head = (int64_t *)calloc((size_t)ngp, sizeof(int64_t)); /* v + 1, 0 = empty (see orc_eval_distances) */
    c.next = (int64_t *)malloc(sizeof(int64_t) * (size_t)ngp);
    c.dist = dist_out;
    c.xp = xp_out;
    init_sampled_planes(g, c.dist, BIG, xp_out);
    {
        int64_t v = 0;
        for (int64_t k = 0; k <= g->N[2]; ++k)
        {
          if (k % g_kstride != g_kphase) { v += (g->N[0] + 1) * (g->N[1] + 1); continue; }
          for (int64_t j = 0; j <= g->N[1]; ++j)
            for (int64_t i = 0; i <= g->N[0]; ++i, ++v) {
                double p[3];
                grid_point(g, i, j, k, p);
                double I1 = cell_of(g, 0, p[0]), I2 = cell_of(g, 1, p[1]), I3 = cell_of(g, 2, p[2]);
                int64_t Ia = (int64_t)(I3 * (double)(g->N[0] + 1) * (double)(g->N[1] + 1) + I2 * (double)(g->N[0] + 1) + I1);
                c.next[v] = c.head[Ia] - 1;
                c.head[Ia] = v + 1;
            }
        }
    }
    int64_t n_solid = 0, n_iso = 0;
    for (int64_t el = 0; el < nel; ++el) {
        double Xe[16][3] = {{0}}, re[16] = {0}, rmin = INFINITY, rmax = -INFINITY; /* 16 rows: shared signatures */
        for (int a = 0; a < 4; ++a) {
            int64_t n = IEN[el * 4 + a] - 1;
            for (int i = 0; i < 3; ++i) Xe[a][i] = X[3 * n + i];
            re[a] = rho_n[n];
            if (re[a] < rmin) rmin = re[a];
            if (re[a] > rmax) rmax = re[a];
        }
        if (rmin >= rho_t) {
            n_solid++;
            process_boundary_faces(&c, &m, el, 1, Xe, re, rho_t);
        } else if (rmax > rho_t) {
            n_iso++;
            process_boundary_faces(&c, &m, el, 0, Xe, re, rho_t);
            int64_t Imin[3], Imax[3];
            mini_aabb(g, Xe, 4, c.delta, Imin, Imax);
            for (int64_t I3 = Imin[2]; I3 <= Imax[2]; ++I3)
              for (int64_t I2 = Imin[1]; I2 <= Imax[1]; ++I2)
                for (int64_t I1 = Imin[0]; I1 <= Imax[0]; ++I1) {
                    int64_t ii = I3 * (g->N[0] + 1) * (g->N[1] + 1) + I2 * (g->N[0] + 1) + I1;
                    for (int64_t v = c.head[ii] - 1; v != -1; v = c.next[v]) {
                        int64_t vi = v % (g->N[0] + 1), vj = (v / (g->N[0] + 1)) % (g->N[1] + 1);
                        int64_t vk = v / ((g->N[0] + 1) * (g->N[1] + 1));
                        double x[3], lam[3], N[4], xp[3], dv[3];
                        grid_point(g, vi, vj, vk, x);
                        iso_project_tet4(x, Xe, re, rho_t, lam);
                        c.n_iso_solves++;
                        tet4_shape(lam, N);
                        for (int i = 0; i < 3; ++i) {
                            double s = 0.0;
                            for (int k = 0; k < 4; ++k) s += Xe[k][i] * N[k];
                            xp[i] = s;
                            dv[i] = x[i] - s;
                        }
                        write_value(&c, v, norm3(dv), xp);
                    }
                }
        }
    }
    if (stats) {
        stats->n_solid = n_solid; stats->n_iso = n_iso; stats->n_iso_solves = c.n_iso_solves;
        stats->n_iso_fail = 0; stats->n_tri_tests = c.n_tri_tests; stats->n_invmap = c.n_invmap;
    }
    free(c.head); free(c.next);
    mesh_free(&m);
    return 0;
}

/* is_point_in_tetrahedron (SignDetection.jl:220-242), tolerance 1e-10 */
static int point_in_tet(const double Xe[8][3], const double mn[3], const double mx[3], const double p[3])
{
    const double tol = 1e-10;
    for (int i = 0; i < 3; ++i)
        if (p[i] < mn[i] - tol || p[i] > mx[i] + tol) return 0;
    double T[16], b[4] = {p[0], p[1], p[2], 1.0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) T[4 * r + c] = Xe[c][r];
    for (int c = 0; c < 4; ++c) T[12 + c] = 1.0;
    if (lu_solve(4, T, b)) return 0;
    for (int i = 0; i < 4; ++i)
        if (!(b[i] >= -tol) || !(b[i] <= 1.0 + tol)) return 0;
    return 1;
}

/* Sign_Detection_TET4 (SignDetection.jl:88-165) with the tetrahedra binned as in
 * create_grid_tetrahedra_mapping_TET4 (:168-217), single thread = ascending element order per bin */
int orc_sign_detection_tet4(const double *X, const int64_t *IEN, int64_t nel, const double *rho_n, double rho_t,
                            const orc_grid *g, double *signs)
{
    int64_t ngp = g->ngp, nx = g->N[0] + 1, ny = g->N[1] + 1, nz = g->N[2] + 1;
    int64_t dims[3] = {nx, ny, nz};
    unsigned char *done = (unsigned char *)calloc((size_t)ngp, 1);
    int64_t *gidx = (int64_t *)malloc(sizeof(int64_t) * 3 * (size_t)ngp);
    {
        int64_t v = 0;
        for (int64_t k = 0; k < nz; ++k) {
          if (k % g_kstride != g_kphase) { v += nx * ny; continue; } /* plane not sampled: never read below */
          for (int64_t j = 0; j < ny; ++j)
            for (int64_t i = 0; i < nx; ++i, ++v) {
                double x[3];
                grid_point(g, i, j, k, x);
                signs[v] = -1.0;
                for (int ax = 0; ax < 3; ++ax) { /* point_to_grid_index (:258-268) */
                    double f = floor((x[ax] - g->amin[ax]) / g->cell) + 1.0;
                    if (f > (double)dims[ax]) f = (double)dims[ax];
                    if (f < 1.0) f = 1.0;
                    gidx[3 * v + ax] = (int64_t)f;
                }
            }
        }
    }
    for (int64_t el = 0; el < nel; ++el) {
        double Xe[8][3] = {{0}}, re[8] = {0}, mn[3], mx[3];
        for (int a = 0; a < 4; ++a) {
            int64_t n = IEN[el * 4 + a] - 1;
            for (int i = 0; i < 3; ++i) {
                Xe[a][i] = X[3 * n + i];
                if (a == 0 || Xe[a][i] < mn[i]) mn[i] = Xe[a][i];
                if (a == 0 || Xe[a][i] > mx[i]) mx[i] = Xe[a][i];
            }
            re[a] = rho_n[n];
        }
        int64_t lo[3], hi[3]; /* 1-based bin ranges (:191-192) */
        for (int ax = 0; ax < 3; ++ax) {
            double a = floor((mn[ax] - g->amin[ax]) / g->cell) - 1.0;
            double b = ceil((mx[ax] - g->amin[ax]) / g->cell) + 1.0;
            if (a < 1.0) a = 1.0;
            if (b > (double)dims[ax]) b = (double)dims[ax];
            lo[ax] = (int64_t)a; hi[ax] = (int64_t)b;
        }
        /* voxels whose bin index lies in the range: lattice index = bin-1 or bin (rounding), scan one wider */
        for (int64_t k = (lo[2] - 2 < 0 ? 0 : lo[2] - 2); k <= hi[2] && k < nz; ++k) {
            if (k % g_kstride != g_kphase) continue;
            for (int64_t j = (lo[1] - 2 < 0 ? 0 : lo[1] - 2); j <= hi[1] && j < ny; ++j)
                for (int64_t i = (lo[0] - 2 < 0 ? 0 : lo[0] - 2); i <= hi[0] && i < nx; ++i) {
                    int64_t v = (k * ny + j) * nx + i;
                    if (done[v]) continue;
                    const int64_t *gi = gidx + 3 * v;
                    if (gi[0] < lo[0] || gi[0] > hi[0] || gi[1] < lo[1] || gi[1] > hi[1] || gi[2] < lo[2] || gi[2] > hi[2]) continue;
                    double x[3], loc[3], N[4];
                    grid_point(g, i, j, k, x);
                    if (!point_in_tet(Xe, mn, mx, x)) continue;
                    if (!find_local_tet4(Xe, x, loc)) continue;
                    tet4_shape(loc, N);
                    double rho = 0.0;
                    for (int q = 0; q < 4; ++q) rho += N[q] * re[q];
                    if (rho >= rho_t) { signs[v] = 1.0; done[v] = 1; }
                }
        }
    }
    free(done); free(gidx);
    return 0;
}

/* calculate_element_volume, TET4 (src/MeshGrid/MeshVolume.jl:75-117): cube Gauss points collapsed onto
 * the unit tetrahedron; calculate_mesh_volume for TET4 meshes */
int orc_mesh_volume_tet4(const double *X, int64_t nnp, const int64_t *IEN, int64_t nel, const double *rho_e,
                         double *V_domain, double *V_frac)
{
    (void)nnp;
    double gp[3], gw[3], dom = 0.0, to = 0.0;
    orc_gauss_legendre(3, gp, gw);
    for (int64_t e = 0; e < nel; ++e) {
        double xe[4][3];
        for (int a = 0; a < 4; ++a)
            for (int i = 0; i < 3; ++i) xe[a][i] = X[3 * (IEN[e * 4 + a] - 1) + i];
        /* J = xe * dN with dN rows (1,0,0),(0,1,0),(0,0,1),(-1,-1,-1) (ShapeFunctions.jl:53-72) */
        double J[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
                for (int a = 0; a < 4; ++a) {
                    double dn = (a == c) ? 1.0 : ((a == 3) ? -1.0 : 0.0);
                    s += xe[a][r] * dn;
                }
                J[r][c] = s;
            }
        double adet = fabs(det3(J)), vol = 0.0;
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 3; ++j)
                for (int i = 0; i < 3; ++i) {
                    double xi = (gp[i] + 1.0) / 2.0;
                    double eta = (gp[j] + 1.0) / 2.0 * (1.0 - xi);
                    double zeta = (gp[k] + 1.0) / 2.0 * (1.0 - xi - eta);
                    if (xi < 0 || eta < 0 || zeta < 0 || xi + eta + zeta > 1.0) continue; /* :97-99 */
                    double jt = (1.0 - xi) * (1.0 - xi) * (1.0 - xi - eta) / 8.0;           /* :108 */
                    vol += gw[i] * gw[j] * gw[k] * adet * jt;
                }
        dom += vol;
        to += vol * rho_e[e];
    }
    *V_domain = dom;
    *V_frac = to / dom;
    return 0;
}
