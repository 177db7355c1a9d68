// exp(-t) of the RBF kernel arguments, shared by the lattice evaluations (r2s_post.hip) and the point evaluator
// (r2s_field.hip): both form their kernel values with the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

// exp(-t) for 0 <= t <= 64 (kernel arguments: t = (dist/sigma)^2 <= -ln(threshold)): t = k ln2/64 + r, exp(-t) =
// 2^(-k/64) exp(-r) with 2^(-j/64) from a 64-entry table and a degree-6 Taylor polynomial of exp(-r), |r| <= ln2/128.
// Relative error <= 2 ulp(Float64) - the class of difference that already separates libm's exp from the device
// library's (the smoothing stage is compared at Float32 round-off) - at a quarter of the device
// library's instruction count; the RBF evaluations spend most of their time in it.
static __constant__ double c_exp2_neg_64[64] = {   // 2^(-j/64), j = 0..63, correctly rounded
    1, 0.98922801319397546, 0.97857206208770009, 0.96803089674614717,
    0.9576032806985737, 0.9472879907934828, 0.93708381705514998, 0.92698956254169274,
    0.91700404320467122, 0.90712608775019943, 0.89735453750155358, 0.88768824626326059,
    0.87812608018664973, 0.86866691763685311, 0.85930964906123897, 0.85005317685926174,
    0.8408964152537145, 0.83183829016336819, 0.82287773907698247, 0.81401371092867392,
    0.80524516597462714, 0.7965710756711335, 0.78799042255394325, 0.77950220011891846,
    0.77110541270397037, 0.76279907537226921, 0.75458221379671142, 0.74645386414563242,
    0.73841307296974967, 0.73045889709032352, 0.72259040348852333, 0.71480666919598501,
    0.70710678118654757, 0.69948983626915562, 0.69195494098191601, 0.68450121148729526,
    0.67712777346844633, 0.66983376202665146, 0.66261832157987066, 0.65548060576238221,
    0.64841977732550482, 0.64143500803938913, 0.63452547859586661, 0.62769037851234555,
    0.620928906036742, 0.61424026805343501, 0.60762367999023448, 0.60107836572635154,
    0.59460355750136051, 0.58819849582514061, 0.58186242938878874, 0.57559461497649134,
    0.56939431737834578, 0.56326080930412092, 0.55719337129794622, 0.55119129165392045,
    0.54525386633262884, 0.53938039887855993, 0.53357020033841185, 0.52782258918027858,
    0.52213689121370688, 0.51651243951061421, 0.51094857432705831, 0.50544464302585024,
};
__device__ __forceinline__ double exp_neg_fast(double t, const double* __restrict__ tab)
{
    const double kf = rint(t * 92.33248261689366);              // 64 / ln 2
    double r = fma(-kf, 0.010830424696248286, t);               // ln2/64, high part (11 trailing zero bits: exact product for k < 2^11)
    r = fma(-kf, 8.59050471673183e-16, r);                      // low part
    const int k = (int)kf;
    double p = fma(r, -1.0 / 720.0, 1.0 / 120.0);
    p = fma(r, -p, 1.0 / 24.0);
    p = fma(r, -p, 1.0 / 6.0);
    p = fma(r, -p, 0.5);
    p = fma(r, -p, 1.0);
    p = fma(r, -p, 1.0);
    return ldexp(tab[k & 63] * p, -(k >> 6));
}
