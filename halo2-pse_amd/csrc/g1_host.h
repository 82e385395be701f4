// g1_host.h -- few-term sums of BN254 G1 points on the calling thread (include/halo2hip_g1.h), over host64.h's 4 x 64 field and XYZZ
// group law.  Host only: no HIP call, no engine state, no lock; the library's entry point and tests/cpp/test_g1_lincomb.cpp share this one
// definition.
//
//   out[j] = addends[j] + sum_{i < t} [scalars[j t + i]] points[i],   j < m
//
// Each sum is one Straus ladder: a doubling chain shared by its t points, an addition wherever a scalar's bit is set.  Every addition is
// h64::padd, which is complete (equal operands double, opposite operands cancel, an identity on either side is returned as it is), so no
// input is exceptional.  Variable-time in the scalars, like every MSM of this library.  All m results reach affine form through one field
// inversion (Montgomery's trick over the results' ZZZ).
#pragma once
#include <stdio.h>

#include <vector>

#include "host64.h"

namespace h2 {
namespace g1h {

static const size_t MAX_TERMS = 4096;  // m * t above this is an MSM's work

static inline h64::F f_one() {
    h64::F o;
    Fe one = fe_one<Q>();
    memcpy(&o, &one, 32);
    return o;
}

// a^(q - 2); 0 -> 0
static inline h64::F f_inv(const h64::F& a) {
    uint64_t e[4];
    memcpy(e, h64::QMOD, 32);
    e[0] -= 2;  // q is odd and its low limb is above 2
    h64::F r = f_one();
    for (int i = 255; i >= 0; i--) {
        r = h64::sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = h64::mul(r, a);
    }
    return r;
}

static inline h64::P from_jacobian(const uint64_t xyz[12]) {
    h64::P o;
    h64::F z;
    memcpy(&z, xyz + 8, 32);
    if (h64::is_zero(z)) return h64::identity();
    memcpy(&o.x, xyz, 32);
    memcpy(&o.y, xyz + 4, 32);
    o.zz = h64::sqr(z);
    o.zzz = h64::mul(o.zz, z);
    return o;
}

// 0, or 1 with the reason in err (the text after "g1_linear_combinations: ")
static inline int linear_combinations(const uint64_t* addends_xyz, const uint64_t* scalars, const uint64_t* points_xy, size_t m, size_t t,
                                      uint64_t* out_xy, char* err, size_t err_len) {
    if (m == 0) return 0;
    if (t && m > MAX_TERMS / t) {
        snprintf(err, err_len, "m = %zu sums of t = %zu terms are more than %zu terms: that is an MSM", m, t, MAX_TERMS);
        return 1;
    }
    if (!out_xy) {
        snprintf(err, err_len, "null out_xy");
        return 1;
    }
    if (t && !scalars) {
        snprintf(err, err_len, "null scalars");
        return 1;
    }
    if (t && !points_xy) {
        snprintf(err, err_len, "null points_xy");
        return 1;
    }
    std::vector<h64::P> points(t);
    for (size_t i = 0; i < t; i++) {
        Affine a;
        memcpy(&a, points_xy + 8 * i, 64);
        if (!fe_is_canonical<Q>(a.x) || !fe_is_canonical<Q>(a.y) || !affine_on_curve(a)) {
            snprintf(err, err_len, "points_xy[%zu] is neither on the curve nor (0, 0)", i);
            return 1;
        }
        points[i] = h64::from_xyzz(xyzz_from_affine(a));
    }
    std::vector<Fe> bits(m * t);  // the scalars as canonical integers
    for (size_t i = 0; i < m * t; i++) {
        Fe s;
        memcpy(&s, scalars + 4 * i, 32);
        if (!fe_is_canonical<FrP>(s)) {
            snprintf(err, err_len, "scalars[%zu] is not a reduced Fr element", i);
            return 1;
        }
        bits[i] = fe_to_canonical<FrP>(s);
    }
    std::vector<h64::P> sums(m);
    for (size_t j = 0; j < m; j++) {
        const Fe* s = bits.data() + j * t;
        int top = -1;  // the highest bit set in any scalar whose point is not the identity
        for (size_t i = 0; i < t; i++) {
            if (h64::is_zero(points[i].zz)) continue;
            for (int b = 255; b > top; b--)
                if ((s[i].l[b >> 5] >> (b & 31)) & 1) top = b;
        }
        h64::P acc = h64::identity();
        for (int b = top; b >= 0; b--) {
            acc = h64::pdouble(acc);
            for (size_t i = 0; i < t; i++)
                if ((s[i].l[b >> 5] >> (b & 31)) & 1) h64::padd(acc, points[i]);
        }
        if (addends_xyz) h64::padd(acc, from_jacobian(addends_xyz + 12 * j));
        sums[j] = acc;
    }
    // x = X / ZZ, y = Y / ZZZ and ZZ^-1 = (ZZ ZZZ^-1)^2: invert the product of the ZZZ once, then peel it from the back
    std::vector<h64::F> prefix(m);
    h64::F run = f_one();
    for (size_t j = 0; j < m; j++) {
        prefix[j] = run;
        if (!h64::is_zero(sums[j].zz)) run = h64::mul(run, sums[j].zzz);
    }
    run = f_inv(run);
    for (size_t j = m; j-- > 0;) {
        uint64_t* o = out_xy + 8 * j;
        if (h64::is_zero(sums[j].zz)) {
            memset(o, 0, 64);
            continue;
        }
        h64::F zi3 = h64::mul(run, prefix[j]);
        run = h64::mul(run, sums[j].zzz);
        h64::F zi2 = h64::sqr(h64::mul(zi3, sums[j].zz));
        h64::F x = h64::mul(sums[j].x, zi2), y = h64::mul(sums[j].y, zi3);
        memcpy(o, &x, 32);
        memcpy(o + 4, &y, 32);
    }
    return 0;
}

}  // namespace g1h
}  // namespace h2
