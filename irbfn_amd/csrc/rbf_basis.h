// The thirteen basis functions (flax_rbf.py:34-111) and their slopes: every formula of a basis in device code stands here, once,
// for float and double.  d = sqrt(sum sq) / sigma (flax_rbf.py:280), u = d2 = d^2, phi = f(u).  The float32 kernels evaluate the
// VALUE of a fast class (common.h) from the record's folded scale (basis_from_r2, rbf_forward.h); all else comes from here.
// Three tables: the slope at d = 0 has two conventions, and the x-VJP wants value and slope from one switch (two switches, or a
// value table derived from the joint one, are 4-10 % more instructions in every generic kernel):
//   basis_value                  phi(d2)
//   basis_slope, _generic, _fast d phi / d(d2) as jax.grad has it (the parameter VJPs): NaN for a query ON a centre
//   basis_value_slope_finite     phi and d phi / d(d2) in the forms that stay finite (the x-VJPs): 0 where the slope diverges
#pragma once

#include "common.h"

namespace irbfn {

template <class T> constexpr T kLog2e = T(1.4426950408889634);       // exp(v) = 2^(kLog2e v)
template <class T> constexpr T kSqrt3 = T(1.7320508075688772);
template <class T> constexpr T kSqrt5 = T(2.23606797749979);
static_assert(kLog2e<float> == 1.4426950408889634f && 2.0f * kLog2e<float> == 2.8853900817779268f &&
              kSqrt3<float> == 1.7320508075688772f && kSqrt5<float> == 2.23606797749979f &&
              float(5) / float(3) == 5.0f / 3.0f && float(5) / float(6) == 5.0f / 6.0f, "the float constants are the f-suffixed literals");

// phi from d2: the generic class; ALL: the fast classes too, in their plain forms (float64 mode)
template <class T, bool ALL = false>
__device__ __forceinline__ T basis_value(T d2, int basis) {
  const T d = sqrt(d2);
  if constexpr (ALL) {
    switch (basis) {
      case IRBFN_GAUSSIAN: return exp(-T(1.0) * d2);
      case IRBFN_GAUSSIAN_WIDE: return exp(-T(0.1) * d2);
      case IRBFN_GAUSSIAN_WIDER: return exp(-T(0.01) * d2);
      case IRBFN_INVERSE_QUADRATIC: return T(1) / (T(1) + d2);
      case IRBFN_INVERSE_MULTIQUADRIC: return T(1) / sqrt(T(1) + d2);
      default: break;
    }
  }
  switch (basis) {
    case IRBFN_LINEAR: return d;                                                        // :55-57
    case IRBFN_QUADRATIC: return d2;                                                    // :61-63
    case IRBFN_MULTIQUADRIC: return sqrt(T(1) + d2);                                    // :67-69
    case IRBFN_SPLINE: return d2 * log(d + T(1));                                       // :79-81
    case IRBFN_POISSON_ONE: return (d - T(1)) * exp(-d);                                // :85-87
    case IRBFN_POISSON_TWO: return ((d - T(2)) / T(2)) * d * exp(-d);                   // :91-97
    case IRBFN_MATERN32: return (T(1) + kSqrt3<T> * d) * exp(-kSqrt3<T> * d);
    case IRBFN_MATERN52: return (T(1) + kSqrt5<T> * d + (T(5) / T(3)) * d2) * exp(-kSqrt5<T> * d);
    default: return T(0);
  }
}

// d phi / d(d2) of the fast classes from phi; gscale: a of exp(-a d2) (gauss_scale, common.h)
template <int BC, class T>
__device__ __forceinline__ T basis_slope_fast(T phi, T gscale) {
  if constexpr (BC == BC_GAUSS) return -gscale * phi;              // exp(-a d2)
  else if constexpr (BC == BC_IQ) return -(phi * phi);             // 1/(1+d2)
  else return -T(0.5) * phi * phi * phi;                           // (1+d2)^-1/2
}

// d phi / d(d2) from phi and d2, parameter-VJP convention.  The bases that depend on d = sqrt(d2) itself have
// d phi / d(d2) = phi'(d) * (0.5 / d), evaluated literally so that a query ON a centre (d = 0) gives what jax.grad gives
// there -- sqrt has no derivative at 0: inf, and inf * 0 = NaN.
// `ls_term` is the factor of the log_sig sum, in the units of `slope * r2` (the caller multiplies the finished sums by
// -2 / sigma^2): for the d-dependent bases it is phi'(d) * d / (2 s2), i.e. d log_sig = phi'(d) * (-d) -- the width does
// NOT go through the sqrt in the reference (flax_rbf.py:280: sqrt(sum sq) / exp(log_sig)), so its gradient is finite (0)
// for a query on a centre, where only the centre path is NaN.
template <class T>
__device__ __forceinline__ T basis_slope_generic(T phi, T d2, T r2, T s2, int basis, T& ls_term) {
  if (basis == IRBFN_MULTIQUADRIC) { const T t = T(0.5) / phi; ls_term = t * r2; return t; }   // sqrt(1+d2)
  if (basis == IRBFN_QUADRATIC) { ls_term = r2; return T(1); }                                  // d2
  const T d = sqrt(d2);
  T dp;                                                        // phi'(d)
  switch (basis) {
    case IRBFN_LINEAR: dp = T(1); break;                                                          // d
    case IRBFN_SPLINE: dp = T(2) * d * log(d + T(1)) + d2 / (d + T(1)); break;                    // d^2 log(d + 1)
    case IRBFN_POISSON_ONE: dp = (T(2) - d) * exp(-d); break;                                     // (d - 1) exp(-d)
    case IRBFN_POISSON_TWO: dp = (T(2) * d - T(1) - T(0.5) * d2) * exp(-d); break;                // ((d - 2) / 2) d exp(-d)
    case IRBFN_MATERN32: dp = -T(3) * d * exp(-kSqrt3<T> * d); break;                             // (1 + sqrt3 d) exp(-sqrt3 d)
    case IRBFN_MATERN52: dp = -(T(5) / T(3)) * d * (T(1) + kSqrt5<T> * d) * exp(-kSqrt5<T> * d); break;   // (1 + sqrt5 d + 5/3 d^2) exp(-sqrt5 d)
    default: dp = T(0); break;
  }
  ls_term = T(0.5) * dp * d / s2;
  return dp * (T(0.5) / d);
}

// the same for a float32 kernel specialised on the basis class BC
template <int BC>
__device__ __forceinline__ float basis_slope(float phi, float d2, float r2, float s2, float gscale, int basis, float& ls_term) {
  if constexpr (BC == BC_GENERIC) {
    return basis_slope_generic(phi, d2, r2, s2, basis, ls_term);
  } else {
    const float t = basis_slope_fast<BC>(phi, gscale);
    ls_term = t * r2;
    return t;
  }
}

// phi (returned) and fprime = d phi / d(d2) from u = d2, x-VJP convention: a query exactly ON a centre contributes 0.  In these
// forms spline / matern32 / matern52 reach their finite limit there; for linear, poisson_one and poisson_two, whose
// f'(u) = phi'(d) / (2 d) diverges at d = 0, the 0 is a convention -- jax.grad gives NaN.
template <class T>
__device__ __forceinline__ T basis_value_slope_finite(T u, int basis, T& fprime) {
  const T d = sqrt(u);
  switch (basis) {
    case IRBFN_LINEAR: fprime = d > T(0) ? T(0.5) / d : (d == T(0) ? T(0) : d); return d;
    case IRBFN_QUADRATIC: fprime = T(1); return u;
    case IRBFN_MULTIQUADRIC: {
      const T p = sqrt(T(1) + u);
      fprime = T(0.5) / p;
      return p;
    }
    case IRBFN_SPLINE: {
      const T l = log(d + T(1));
      fprime = l + T(0.5) * d / (d + T(1));
      return u * l;
    }
    case IRBFN_POISSON_ONE: {
      const T e = exp(-d);
      fprime = d > T(0) ? (T(2) - d) * e * (T(0.5) / d) : (d == T(0) ? T(0) : d);
      return (d - T(1)) * e;
    }
    case IRBFN_POISSON_TWO: {
      const T e = exp(-d);
      fprime = d > T(0) ? (T(2) * d - T(1) - T(0.5) * u) * e * (T(0.5) / d) : (d == T(0) ? T(0) : d);
      return ((d - T(2)) / T(2)) * d * e;
    }
    case IRBFN_MATERN32: {
      const T e = exp(-kSqrt3<T> * d);
      fprime = -T(1.5) * e;
      return (T(1) + kSqrt3<T> * d) * e;
    }
    case IRBFN_MATERN52: {
      const T e = exp(-kSqrt5<T> * d);
      fprime = -(T(5) / T(6)) * (T(1) + kSqrt5<T> * d) * e;
      return (T(1) + kSqrt5<T> * d + (T(5) / T(3)) * u) * e;
    }
    default: fprime = T(0); return T(0);
  }
}

}  // namespace irbfn
