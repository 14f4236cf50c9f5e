// sinpi.h — sin(pi t) and cos(pi t) for the Periodic leaf (periodic.jl:45-52), shared by cov.hip and grad.hip.
//
// The leaf only needs sin^2(pi t) and sin(2 pi t) = 2 sin(pi t) cos(pi t), both of period 1 in t, so the argument is reduced in
// the PERIOD domain: u = t - rint(t), |u| <= 1/2.  That subtraction is exact (t and rint(t) are within a factor of two of each
// other once rint(t) != 0), so no digits of pi enter the reduction — unlike sin(pi * r / p) in the reference, whose product
// rounds before sin (about 1.6e-14 absolute at r/p ~ 46).  The sign (-1)^rint(t) that the reduction drops cancels in both uses.
// fp64: odd / even Taylor polynomials of pi u, Horner in u^2 with the constants in scalar registers (the pattern of exp_nonpos,
// cov.hip) — no library sin, no Payne-Hanek path.  On |u| <= 1/2 the first omitted terms are (pi/2)^23 / 23! = 1.3e-18 (sin) and
// (pi/2)^24 / 24! = 8.2e-20 (cos); with Horner's rounding |abs. error| < 2.5e-16 for both.  What remains is the input's own error:
// t = r/p carries |t| * 2^-52 from the distance and the root, which becomes pi |t| 2^-52 in the sine (6e-15 at t = 10).
// fp32: sinf / cosf on the reduced argument.
#pragma once
#include <hip/hip_runtime.h>

namespace gpmi {

__device__ __forceinline__ double sinpi_poly(double u) {  // sin(pi u), |u| <= 1/2
    const double u2 = u * u;
    double p = 5.392664662608129e-10;       //  pi^21 / 21!
    p = fma(p, u2, -2.2948428997269873e-08);  // -pi^19 / 19!
    p = fma(p, u2, 7.952054001475513e-07);    //  pi^17 / 17!
    p = fma(p, u2, -2.1915353447830217e-05);  // -pi^15 / 15!
    p = fma(p, u2, 4.6630280576761255e-04);   //  pi^13 / 13!
    p = fma(p, u2, -7.3704309457143504e-03);  // -pi^11 / 11!
    p = fma(p, u2, 8.214588661112823e-02);    //  pi^9 / 9!
    p = fma(p, u2, -5.992645293207921e-01);   // -pi^7 / 7!
    p = fma(p, u2, 2.5501640398773455);       //  pi^5 / 5!
    p = fma(p, u2, -5.16771278004997);        // -pi^3 / 3!
    p = fma(p, u2, 3.141592653589793);        //  pi
    return p * u;
}
__device__ __forceinline__ double cospi_poly(double u) {  // cos(pi u), |u| <= 1/2
    const double u2 = u * u;
    double p = -7.700707130601354e-11;      // -pi^22 / 22!
    p = fma(p, u2, 3.604730797462501e-09);    //  pi^20 / 20!
    p = fma(p, u2, -1.3878952462213771e-07);  // -pi^18 / 18!
    p = fma(p, u2, 4.303069587032947e-06);    //  pi^16 / 16!
    p = fma(p, u2, -1.046381049248457e-04);   // -pi^14 / 14!
    p = fma(p, u2, 1.9295743094039231e-03);   //  pi^12 / 12!
    p = fma(p, u2, -2.580689139001406e-02);   // -pi^10 / 10!
    p = fma(p, u2, 2.353306303588932e-01);    //  pi^8 / 8!
    p = fma(p, u2, -1.3352627688545895);      // -pi^6 / 6!
    p = fma(p, u2, 4.0587121264167685);       //  pi^4 / 4!
    p = fma(p, u2, -4.934802200544679);       // -pi^2 / 2!
    return fma(p, u2, 1.0);
}

// sin(pi (t - rint t)): its square is sin^2(pi t)
__device__ __forceinline__ double sinpi_mod1(double t) { return sinpi_poly(t - rint(t)); }
__device__ __forceinline__ float sinpi_mod1(float t) { return sinf(3.14159265358979f * (t - rintf(t))); }

// sin and cos of pi (t - rint t): 2 sn cs = sin(2 pi t)
__device__ __forceinline__ void sincospi_mod1(double t, double* sn, double* cs) {
    const double u = t - rint(t);
    *sn = sinpi_poly(u);
    *cs = cospi_poly(u);
}
__device__ __forceinline__ void sincospi_mod1(float t, float* sn, float* cs) {
    const float u = 3.14159265358979f * (t - rintf(t));
    *sn = sinf(u);
    *cs = cosf(u);
}

}  // namespace gpmi
