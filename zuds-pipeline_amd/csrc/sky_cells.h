// Geometry shared by associate.hip and skyindex.hip (gfx950): fp64 unit vectors binned into cubic cells whose edge is the
// chord of a radius times 1 + 1e-6, and the 64-bit key and hash of a cell.  Both units must use exactly this arithmetic:
// a k = 1 query of the resident index returns the bits zm_crossmatch returns.
#pragma once
#include "zm_internal.h"

typedef unsigned long long as_u64;

#define AS_EMPTY (~0ull)              // no key has bit 63 set: three fields of 21 bits
#define AS_OFF (1ll << 20)            // cell coordinates are stored + AS_OFF, in [0, 2^21)
#define AS_ARCSEC_PER_RAD (648000.0 / 3.14159265358979323846)

struct as_grid {
    double edge;                      // cell edge: chord(r) * (1 + 1e-6)
    double thr;                       // (2 sin(r / 2))^2
    as_u64 mask;                      // capacity - 1
};

__device__ __forceinline__ bool as_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__device__ __forceinline__ long long as_cell(double v, double edge) { return (long long)floor(v / edge); }

__device__ __forceinline__ as_u64 as_key(long long cx, long long cy, long long cz) {
    return ((as_u64)(cx + AS_OFF) << 42) | ((as_u64)(cy + AS_OFF) << 21) | (as_u64)(cz + AS_OFF);
}

__device__ __forceinline__ as_u64 as_hash(as_u64 k) {          // (the finaliser of splitmix64)
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k;
}

__device__ __forceinline__ void as_unit(double ra_deg, double dec_deg, double* x, double* y, double* z) {
    const double d2r = 3.14159265358979323846 / 180.0;
    const double ra = ra_deg * d2r, dec = dec_deg * d2r;
    const double cd = cos(dec);
    *x = cd * cos(ra);
    *y = cd * sin(ra);
    *z = sin(dec);
}
