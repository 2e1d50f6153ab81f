// Training augmentation on the device (neurovit_amd.augment.VolumeAugment): a per-sample random crop (monai's RandSpatialCrop with a fixed
// size, the reference's DATASET_TRANSFORMS switch), integer translation, axis flips and an affine intensity change, for 3D volumes and
// 4D series.  Every sample has its own offset, so the crop is no strided view: one streaming pass copies it.
//
//   nv_augment_params   (config, seed, step, rank) -> params int32 [B, 8]: {ox, oy, oz, flip bits, bits of scale, bits of shift, 0, 0},
//                       drawn on the device with nv_hash64 (the rule is in the header; tests/augment_ref.py restates it)
//   nv_augment_apply    src fp32 [B, X, Y, Z, T] (any strides) + params -> out fp32 [B, Sx, Sy, Sz, T] dense
//
// The copy is laid out like nv_mask_patches: a workgroup owns AG_SPAN consecutive elements of one output plane (b, i) - Sy Sz T contiguous
// floats - so the grid follows the rows, not the batch; the 16-byte groups follow the alignment of the plane in `out` (split_span).  A
// group whose four cells lie in one source row that is contiguous in memory is read with one 16-byte load when the address allows it
// (load4), backwards under a z flip of a 3D volume; every other group (row ends, window edges, strided sources, a flipped series) is
// gathered cell by cell.  Voxels move as 32-bit patterns and the intensity change is two separately rounded operations (contraction is
// off for the whole file), skipped altogether for scale 1 / shift 0: that sample is a bit copy.  No atomics, every output element is
// written once by one thread.
#include "attr_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int AG_THREADS = 256;
constexpr int AG_SPAN = 4096;            // elements of one output plane a workgroup owns: four 16-byte groups per thread

// ------------------------------------------------------------------------------------------------ parameters
struct AugDraw {
  unsigned crop_n[3];                    // X - Sx + 1: the crop offset is uniform on [0, crop_n)
  int max_shift[3];
  unsigned flip_thresh[3];               // (unsigned)(p * 65536)
  float scale_lo, scale_hi, shift_lo, shift_hi;
};

__device__ __forceinline__ int draw_below(uint64_t h, unsigned n) { return (int)(((h >> 32) * (uint64_t)n) >> 32); }
__device__ __forceinline__ float draw_between(uint64_t h, float lo, float hi) {
  const float u = (float)(unsigned)(h >> 40) * 0x1p-24f;   // 24 bits: exact
  const float width = hi - lo;
  const float part = width * u;
  return lo + part;
}

// One thread per sample: draw d of sample b at step s hashes the counter ((s 2^32 + b) 16 + d) mod 2^64 under the rank's seed.
__global__ __launch_bounds__(AG_THREADS) void augment_params_kernel(AugDraw cfg, uint64_t seed, uint64_t step, uint64_t rank, int B, int* __restrict__ params) {
  const int b = blockIdx.x * AG_THREADS + threadIdx.x;
  if (b >= B) return;
  const uint64_t seed_r = nv_hash64(seed, rank);
  const uint64_t counter = ((step << 32) + (uint64_t)b) * 16u;
  int row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int crop = draw_below(nv_hash64(seed_r, counter + a), cfg.crop_n[a]);
    const int move = draw_below(nv_hash64(seed_r, counter + 3 + a), 2u * (unsigned)cfg.max_shift[a] + 1u) - cfg.max_shift[a];
    row[a] = crop + move;
    if ((unsigned)(nv_hash64(seed_r, counter + 6 + a) >> 48) < cfg.flip_thresh[a]) row[3] |= 1 << a;
  }
  row[4] = __float_as_int(draw_between(nv_hash64(seed_r, counter + 9), cfg.scale_lo, cfg.scale_hi));
  row[5] = __float_as_int(draw_between(nv_hash64(seed_r, counter + 10), cfg.shift_lo, cfg.shift_hi));
#pragma unroll
  for (int i = 0; i < 8; ++i) params[8L * b + i] = row[i];
}

// ------------------------------------------------------------------------------------------------ apply
struct AugGeom {
  int X, Y, Z, T, Sx, Sy, Sz;
  long st_b, st_x, st_y, st_z, st_t;     // element strides of src
};

// Grid (B Sx, ceil(Sy Sz T / AG_SPAN)).  The offsets of a parameter row may be anything: every read is bounds-checked against the volume,
// and a cell outside it gets `fill`.
__global__ __launch_bounds__(AG_THREADS) void augment_apply_kernel(const unsigned* __restrict__ src, AugGeom g, const int* __restrict__ params, unsigned fill,
                                                                   unsigned* __restrict__ out) {
  const int tid = threadIdx.x;
  const int plane = blockIdx.x, b = plane / g.Sx, i = plane - b * g.Sx;
  const int T = g.T, L = g.Sz * T, P = g.Sy * L;           // cells of one output row (j) and of the plane
  const int e0 = blockIdx.y * AG_SPAN, len = min(AG_SPAN, P - e0);
  const int* row = params + 8L * b;
  const long ox = row[0], oy = row[1], oz = row[2];
  const bool fx = row[3] & 1, fy = row[3] & 2, fz = row[3] & 4;
  const float scale = __int_as_float(row[4]), shift = __int_as_float(row[5]);
  const bool copy = scale == 1.0f && shift == 0.0f;
  const long first = (long)plane * P + e0;
  unsigned* o = out + first;
  const Span s = split_span(first, len);
  const u32x4 fill4 = {fill, fill, fill, fill};
  const long sx = ox + (fx ? g.Sx - 1 - i : i);
  if (sx < 0 || sx >= g.X) {                               // (uniform over the workgroup) the whole plane lies outside the volume
    for (int e = tid; e < s.head; e += AG_THREADS) o[e] = fill;
    for (int e = s.tail + tid; e < len; e += AG_THREADS) o[e] = fill;
    for (int q = tid; q < s.groups; q += AG_THREADS) *reinterpret_cast<u32x4*>(o + s.head + 4 * q) = fill4;
    return;
  }
  const unsigned* xp = src + (long)b * g.st_b + sx * g.st_x;
  auto shade = [&](unsigned u) {
    if (copy) return u;
    const float m = __uint_as_float(u) * scale;
    return __float_as_uint(m + shift);
  };
  auto cell = [&](int j, int c) {                          // output cell (j, c = k T + t) of this plane
    const int k = T > 1 ? c / T : c, t = c - k * T;
    const long sy = oy + (fy ? g.Sy - 1 - j : j), sz = oz + (fz ? g.Sz - 1 - k : k);
    if (sy < 0 || sy >= g.Y || sz < 0 || sz >= g.Z) return fill;
    return shade(xp[sy * g.st_y + sz * g.st_z + t * g.st_t]);
  };
  auto single = [&](int e) {
    const int j = (e0 + e) / L;
    o[e] = cell(j, (e0 + e) - j * L);
  };
  for (int e = tid; e < s.head; e += AG_THREADS) single(e);
  for (int e = s.tail + tid; e < len; e += AG_THREADS) single(e);
  // a source row is one run of memory: ascending for a series with time innermost, in either direction for a volume
  const bool run = T > 1 ? (g.st_t == 1 && g.st_z == T && !fz) : g.st_z == 1;
  const long row_cells = (long)g.Z * T;
  for (int q = tid; q < s.groups; q += AG_THREADS) {
    const int e = s.head + 4 * q;
    int j = (e0 + e) / L, c = (e0 + e) - j * L;
    u32x4 v;
    bool done = false;
    if (run && c + 3 < L) {                                // the four cells share the output row j
      const long sy = oy + (fy ? g.Sy - 1 - j : j);
      if (sy < 0 || sy >= g.Y) {
        v = fill4;
        done = true;
      } else {
        const long lowest = fz ? oz + (g.Sz - 1 - c) - 3 : oz * T + c;       // source cell of the group's lowest address
        if (lowest >= 0 && lowest + 3 < row_cells) {
          const unsigned* p = xp + sy * g.st_y + lowest;
          const u32x4 w = load4(p, is_aligned16(p));
          v = fz ? u32x4{w[3], w[2], w[1], w[0]} : w;
#pragma unroll
          for (int m = 0; m < 4; ++m) v[m] = shade(v[m]);
          done = true;
        }
      }
    }
    if (!done) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        v[m] = cell(j, c);
        if (++c == L) { c = 0; ++j; }                      // (a group may straddle rows; j < Sy for every cell that is read, since e + m < len)
      }
    }
    *reinterpret_cast<u32x4*>(o + e) = v;
  }
}
}  // namespace

extern "C" int nv_augment_params(const nv_augment_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* params, void* stream) {
  NV_CHECK_ARG(cfg && params && B > 0 && rank >= 0, "nv_augment_params: bad arguments (null pointer, B not positive or a negative rank)");
  NV_CHECK_ARG(cfg->struct_size == (int)sizeof(nv_augment_config), "nv_augment_params: struct_size %d, this library's nv_augment_config has %d bytes",
               cfg->struct_size, (int)sizeof(nv_augment_config));
  NV_CHECK_ARG(nv_aligned(params, 4), "nv_augment_params: params 4-byte aligned");
  AugDraw d;
  for (int a = 0; a < 3; ++a) {
    const int X = cfg->in_size[a], S = cfg->roi[a], m = cfg->max_shift[a];
    const double p = cfg->flip_prob[a];
    NV_CHECK_ARG(S > 0 && X > 0, "nv_augment_params: axis %d: input %d and roi %d must be positive", a, X, S);
    NV_CHECK_ARG(S <= X, "nv_augment_params: axis %d: roi %d is larger than the input %d", a, S, X);
    NV_CHECK_ARG(m >= 0 && m < (1 << 30), "nv_augment_params: axis %d: max_shift %d outside [0, 2^30)", a, m);
    NV_CHECK_ARG(p >= 0.0 && p <= 1.0, "nv_augment_params: axis %d: flip probability %g outside [0, 1]", a, p);
    d.crop_n[a] = (unsigned)(X - S) + 1u;
    d.max_shift[a] = m;
    d.flip_thresh[a] = (unsigned)(p * 65536.0);
  }
  NV_CHECK_ARG(cfg->scale_lo <= cfg->scale_hi && cfg->shift_lo <= cfg->shift_hi && isfinite(cfg->scale_lo) && isfinite(cfg->scale_hi) &&
                   isfinite(cfg->shift_lo) && isfinite(cfg->shift_hi),
               "nv_augment_params: intensity ranges must be finite with lo <= hi (scale [%g, %g], shift [%g, %g])", cfg->scale_lo, cfg->scale_hi,
               cfg->shift_lo, cfg->shift_hi);
  d.scale_lo = cfg->scale_lo; d.scale_hi = cfg->scale_hi; d.shift_lo = cfg->shift_lo; d.shift_hi = cfg->shift_hi;
  hipLaunchKernelGGL(augment_params_kernel, dim3((B + AG_THREADS - 1) / AG_THREADS), dim3(AG_THREADS), 0, (hipStream_t)stream, d, (uint64_t)seed,
                     (uint64_t)step, (uint64_t)rank, B, params);
  NV_CHECK_LAUNCH("nv_augment_params");
  return NV_OK;
}

extern "C" int nv_augment_apply(const float* src, const long* strides5, int B, const int* in3, int T, const int* params, const int* roi3, float fill,
                                float* out, void* stream) {
  NV_CHECK_ARG(src && strides5 && in3 && params && roi3 && out && B > 0 && T > 0, "nv_augment_apply: bad arguments (null pointer, or B / T not positive)");
  AugGeom g;
  g.X = in3[0]; g.Y = in3[1]; g.Z = in3[2]; g.T = T; g.Sx = roi3[0]; g.Sy = roi3[1]; g.Sz = roi3[2];
  NV_CHECK_ARG(g.X > 0 && g.Y > 0 && g.Z > 0 && g.Sx > 0 && g.Sy > 0 && g.Sz > 0, "nv_augment_apply: input %d x %d x %d and roi %d x %d x %d must be positive",
               g.X, g.Y, g.Z, g.Sx, g.Sy, g.Sz);
  NV_CHECK_ARG(g.Sx <= g.X && g.Sy <= g.Y && g.Sz <= g.Z, "nv_augment_apply: roi %d x %d x %d is larger than the input %d x %d x %d", g.Sx, g.Sy, g.Sz, g.X,
               g.Y, g.Z);
  const long planes = (long)B * g.Sx, P = (long)g.Sy * g.Sz * T, spans = (P + AG_SPAN - 1) / AG_SPAN;
  NV_CHECK_ARG(planes < (1L << 31) && spans <= 65535 && (long)g.Z * T < (1L << 31),
               "nv_augment_apply: %ld output planes of %ld cells beyond one launch (at most 2^31 - 1 planes of %ld cells)", planes, P, 65535L * AG_SPAN);
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned(src, 4) && nv_aligned(params, 4), "nv_augment_apply: out 16-byte aligned, src and params 4-byte aligned");
  g.st_b = strides5[0]; g.st_x = strides5[1]; g.st_y = strides5[2]; g.st_z = strides5[3]; g.st_t = strides5[4];
  union { float f; unsigned u; } fbits;
  fbits.f = fill;
  hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)planes, (unsigned)spans), dim3(AG_THREADS), 0, (hipStream_t)stream, (const unsigned*)src, g, params,
                     fbits.u, (unsigned*)out);
  NV_CHECK_LAUNCH("nv_augment_apply");
  return NV_OK;
}
