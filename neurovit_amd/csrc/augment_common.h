// What the augmentation kernels (augment.hip, affine.hip, mix.hip) share: the draw rule, the fp32 intensity change, the geometry and work
// split of a streaming pass, and the host-side checks of their entry points.  The draw rule and the intensity change are part of the
// C-ABI (include/neurovit_hip.h), and an integer row of nv_affine_apply is bit for bit what nv_augment_apply writes: kernels that must
// agree call the one definition here.  The .hip files switch contraction off AFTER their includes, which does not reach this header, so
// every helper here that does floating-point arithmetic carries the pragma in its own body.
#pragma once
#include "attr_common.h"

constexpr int PASS_THREADS = 256;
constexpr int PASS_SPAN = 4096;          // elements of one output plane a workgroup owns: four 16-byte groups per thread

// ------------------------------------------------------------------------------------------------ draws
// Counter strides and hash domains of the three transforms (ABI: the header states them)
constexpr unsigned AUGMENT_STRIDE = 16, AFFINE_STRIDE = 32, MIX_STRIDE = 256;
constexpr uint64_t AUGMENT_DOMAIN = 0, AFFINE_DOMAIN = 0x414646ull, MIX_DOMAIN = 0x4D4958ull;       // 0: the rank's seed itself

// The draws of sample b at step s: draw d is the hash of the counter ((s 2^32 + b) stride + d) mod 2^64 under the rank's seed in the
// transform's domain
struct SampleDraws {
  uint64_t seed, counter;
  __device__ __forceinline__ SampleDraws(uint64_t seed0, uint64_t rank, uint64_t domain, unsigned stride, uint64_t step, int b) {
    const uint64_t seed_r = nv_hash64(seed0, rank);
    seed = domain ? nv_hash64(seed_r, domain) : seed_r;
    counter = ((step << 32) + (uint64_t)b) * stride;
  }
  __device__ __forceinline__ uint64_t operator()(unsigned d) const { return nv_hash64(seed, counter + d); }
};

// uniform on [0, n), 0 < n < 2^32 (n is 64 bits wide so that a caller's count, int or unsigned, widens in its own way: mix_params_kernel
// hands in an int, and a cast to unsigned in front of the product changes its instructions, though none of its results)
__device__ __forceinline__ int draw_below(uint64_t h, uint64_t n) { return (int)(((h >> 32) * n) >> 32); }
__device__ __forceinline__ float draw_between(uint64_t h, float lo, float hi) {
#pragma clang fp contract(off)
  const float u = (float)(unsigned)(h >> 40) * 0x1p-24f;   // 24 bits: exact
  const float width = hi - lo;
  const float part = width * u;
  return lo + part;
}
// An event of probability p happens when the top 16 bits of its draw lie below (unsigned)(p * 65536)
static inline unsigned chance_thresh(double p) { return (unsigned)(p * 65536.0); }
__device__ __forceinline__ bool draw_chance(uint64_t h, unsigned thresh) { return (unsigned)(h >> 48) < thresh; }

// ------------------------------------------------------------------------------------------------ the pass
struct PassGeom {
  int B, X, Y, Z, T, Sx, Sy, Sz;
  long st_b, st_x, st_y, st_z, st_t;     // element strides of src
};

// A sample's intensity change v * scale + shift, two separately rounded operations; scale 1 / shift 0 is a bit copy
struct Intensity {
  float scale, shift;
  bool copy;

  // (after scale and shift are written)
  __device__ __forceinline__ void settle() { copy = scale == 1.0f && shift == 0.0f; }
  __device__ __forceinline__ unsigned shade(unsigned u) const {
#pragma clang fp contract(off)
    if (copy) return u;
    const float m = __uint_as_float(u) * scale;
    return __float_as_uint(m + shift);
  }
};

// ------------------------------------------------------------------------------------------------ host side
// The checks, the geometry and the launch shape that the pass entry points share.  `who` is the entry point and `tables` its word for
// the parameter rows, for the messages; `rows` must be there, `more` (a second table) may be NULL.
struct PassLaunch {
  PassGeom g;
  dim3 grid;                             // (B Sx, ceil(Sy Sz T / PASS_SPAN))
  unsigned fill;                         // the bits of the fill value
};
static inline int pass_setup(const char* who, const char* tables, const float* src, const long* strides5, int B, const int* in3, int T, const int* rows,
                             const int* more, const int* roi3, float fill, const float* out, PassLaunch& l) {
  NV_CHECK_ARG(src && strides5 && in3 && rows && roi3 && out && B > 0 && T > 0, "%s: bad arguments (null pointer, or B / T not positive)", who);
  PassGeom& g = l.g;
  g.B = B; g.X = in3[0]; g.Y = in3[1]; g.Z = in3[2]; g.T = T; g.Sx = roi3[0]; g.Sy = roi3[1]; g.Sz = roi3[2];
  NV_CHECK_ARG(g.X > 0 && g.Y > 0 && g.Z > 0 && g.Sx > 0 && g.Sy > 0 && g.Sz > 0, "%s: input %d x %d x %d and roi %d x %d x %d must be positive", who, g.X, g.Y,
               g.Z, g.Sx, g.Sy, g.Sz);
  NV_CHECK_ARG(g.Sx <= g.X && g.Sy <= g.Y && g.Sz <= g.Z, "%s: roi %d x %d x %d is larger than the input %d x %d x %d", who, g.Sx, g.Sy, g.Sz, g.X, g.Y, g.Z);
  const long planes = (long)B * g.Sx, P = (long)g.Sy * g.Sz * T, spans = (P + PASS_SPAN - 1) / PASS_SPAN;
  NV_CHECK_ARG(planes < (1L << 31) && spans <= 65535 && (long)g.Z * T < (1L << 31),
               "%s: %ld output planes of %ld cells beyond one launch (at most 2^31 - 1 planes of %ld cells)", who, planes, P, 65535L * PASS_SPAN);
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned(src, 4) && nv_aligned(rows, 4) && nv_aligned(more, 4), "%s: out 16-byte aligned, src and %s 4-byte aligned", who,
               tables);
  g.st_b = strides5[0]; g.st_x = strides5[1]; g.st_y = strides5[2]; g.st_z = strides5[3]; g.st_t = strides5[4];
  l.grid = dim3((unsigned)planes, (unsigned)spans);
  union { float f; unsigned u; } fbits;
  fbits.f = fill;
  l.fill = fbits.u;
  return NV_OK;
}

// What nv_augment_config and nv_affine_config share - per axis in_size, roi and flip_prob, and the two intensity ranges - checked and
// turned into the fields of the same names of the kernel's draw record d
template <typename Config, typename Draw>
static inline int window_draw_setup(const char* who, const Config& cfg, Draw& d) {
  for (int a = 0; a < 3; ++a) {
    const int X = cfg.in_size[a], S = cfg.roi[a];
    const double p = cfg.flip_prob[a];
    NV_CHECK_ARG(S > 0 && X > 0, "%s: axis %d: input %d and roi %d must be positive", who, a, X, S);
    NV_CHECK_ARG(S <= X, "%s: axis %d: roi %d is larger than the input %d", who, a, S, X);
    NV_CHECK_ARG(p >= 0.0 && p <= 1.0, "%s: axis %d: flip probability %g outside [0, 1]", who, a, p);
    d.crop_n[a] = (unsigned)(X - S) + 1u;  // the crop offset is uniform on [0, X - S]
    d.flip_thresh[a] = chance_thresh(p);
  }
  NV_CHECK_ARG(cfg.scale_lo <= cfg.scale_hi && cfg.shift_lo <= cfg.shift_hi && isfinite(cfg.scale_lo) && isfinite(cfg.scale_hi) && isfinite(cfg.shift_lo) &&
                   isfinite(cfg.shift_hi),
               "%s: intensity ranges must be finite with lo <= hi (scale [%g, %g], shift [%g, %g])", who, cfg.scale_lo, cfg.scale_hi, cfg.shift_lo, cfg.shift_hi);
  d.scale_lo = cfg.scale_lo; d.scale_hi = cfg.scale_hi; d.shift_lo = cfg.shift_lo; d.shift_hi = cfg.shift_hi;
  return NV_OK;
}
