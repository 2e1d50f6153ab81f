// Training augmentation on the device (neurovit_amd.augment.VolumeAugment): a per-sample random crop (monai's RandSpatialCrop with a fixed
// size, the reference's DATASET_TRANSFORMS switch), integer translation, axis flips and an affine intensity change, for 3D volumes and
// 4D series, and Mixup / CutMix (neurovit_amd.augment.VolumeMix) fused with it.  Every sample has its own offset, so the crop is no
// strided view: one streaming pass copies it, and a mixed batch is still read once and written once.
//
//   nv_augment_params   (config, seed, step, rank) -> params int32 [B, 8]: {ox, oy, oz, flip bits, bits of scale, bits of shift, 0, 0},
//                       drawn on the device with nv_hash64 (the rule is in the header; tests/augment_ref.py restates it)
//   nv_augment_apply    src fp32 [B, X, Y, Z, T] (any strides) + params -> out fp32 [B, Sx, Sy, Sz, T] dense: A_b, sample b under its row
//   nv_augment_mix      the same + mix rows (nv_mix_params, mix.hip; the augmentation rows may be missing) -> out = A_b, (lambda A_b) +
//                       (mu A_p), or A_p inside the box and A_b outside, each sample under its OWN row
//
// Both are one pass body (augment_pass), laid out like nv_mask_patches: a workgroup owns PASS_SPAN consecutive elements of one output plane
// (b, i) - Sy Sz T contiguous floats - so the grid follows the rows, not the batch; the 16-byte groups follow the alignment of the plane
// in `out` (split_span).  A group whose four cells lie in one source row that is contiguous in memory is read with one 16-byte load when
// the address allows it (load4), backwards under a z flip of a 3D volume; every other group (row ends, window edges, strided sources, a
// flipped series) is gathered cell by cell.  A sample and its partner have rows of their own, so each side decides on its own whether a
// group is one load.  A CutMix group in a row outside the box is the sample's own; in a row that crosses the box both sides' groups are
// fetched and every cell takes its side (x and y are uniform over a group, z is not).  Voxels move as 32-bit patterns; the intensity
// change and the Mixup blend are separately rounded operations (contraction is off for the whole file), the intensity change skipped
// altogether for scale 1 / shift 0: that sample is a bit copy.  No atomics, every output element is written once by one thread.
// The draw rule, the intensity change, the geometry and the host-side checks are those of affine.hip and mix.hip: augment_common.h.
#include "augment_common.h"

#pragma clang fp contract(off)

namespace {
// ------------------------------------------------------------------------------------------------ parameters
struct AugDraw {
  unsigned crop_n[3];                    // X - Sx + 1: the crop offset is uniform on [0, crop_n)
  int max_shift[3];
  unsigned flip_thresh[3];               // (unsigned)(p * 65536)
  float scale_lo, scale_hi, shift_lo, shift_hi;
};

// One thread per sample: draw d of sample b at step s hashes the counter ((s 2^32 + b) 16 + d) mod 2^64 under the rank's seed.
__global__ __launch_bounds__(PASS_THREADS) void augment_params_kernel(AugDraw cfg, uint64_t seed, uint64_t step, uint64_t rank, int B, int* __restrict__ params) {
  const int b = blockIdx.x * PASS_THREADS + threadIdx.x;
  if (b >= B) return;
  const SampleDraws h(seed, rank, AUGMENT_DOMAIN, AUGMENT_STRIDE, step, b);
  int row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int crop = draw_below(h(a), cfg.crop_n[a]);
    const int move = draw_below(h(3 + a), 2u * (unsigned)cfg.max_shift[a] + 1u) - cfg.max_shift[a];
    row[a] = crop + move;
    if (draw_chance(h(6 + a), cfg.flip_thresh[a])) row[3] |= 1 << a;
  }
  row[4] = __float_as_int(draw_between(h(9), cfg.scale_lo, cfg.scale_hi));
  row[5] = __float_as_int(draw_between(h(10), cfg.shift_lo, cfg.shift_hi));
#pragma unroll
  for (int i = 0; i < 8; ++i) params[8L * b + i] = row[i];
}

// ------------------------------------------------------------------------------------------------ the pass
// What the pass writes for one sample on output plane i: the cells of A_s, singly or four at a time.  The offsets of a parameter row
// may be anything: every read is bounds-checked against the volume, and a cell outside it gets `fill`.
struct Side {
  const unsigned* xp;                    // the source plane (valid when plane_in)
  long oy, oz;
  bool fy, fz, plane_in, run;
  Intensity tone;
  unsigned fill;

  __device__ __forceinline__ void init(const unsigned* src, const PassGeom& g, const int* aug, int s, int i, unsigned fill_bits) {
    long ox = 0;
    int flips = 0;
    oy = 0; oz = 0; tone.scale = 1.0f; tone.shift = 0.0f;
    if (aug) {                                             // (a NULL table is identity rows)
      const int* row = aug + 8L * s;
      ox = row[0]; oy = row[1]; oz = row[2]; flips = row[3];
      tone.scale = __int_as_float(row[4]); tone.shift = __int_as_float(row[5]);
    }
    fy = flips & 2; fz = flips & 4;
    tone.settle();
    fill = fill_bits;
    const long sx = ox + ((flips & 1) ? g.Sx - 1 - i : i);
    plane_in = sx >= 0 && sx < g.X;
    xp = src + (long)s * g.st_b + (plane_in ? sx : 0) * g.st_x;
    // a source row is one run of memory: ascending for a series with time innermost, in either direction for a volume
    run = g.T > 1 ? (g.st_t == 1 && g.st_z == g.T && !fz) : g.st_z == 1;
  }
  // output cell (j, k, t) of the plane
  __device__ __forceinline__ unsigned cell(const PassGeom& g, int j, int k, int t) const {
    const long sy = oy + (fy ? g.Sy - 1 - j : j), sz = oz + (fz ? g.Sz - 1 - k : k);
    if (!plane_in || sy < 0 || sy >= g.Y || sz < 0 || sz >= g.Z) return fill;
    return tone.shade(xp[sy * g.st_y + sz * g.st_z + t * g.st_t]);
  }
  // the four cells c .. c + 3 of output row j (c + 3 < Sz T): one 16-byte load where the source allows it
  __device__ __forceinline__ u32x4 group(const PassGeom& g, int j, int c) const {
    const int T = g.T;
    if (run) {
      const long sy = oy + (fy ? g.Sy - 1 - j : j);
      if (!plane_in || sy < 0 || sy >= g.Y) return u32x4{fill, fill, fill, fill};
      const long lowest = fz ? oz + (g.Sz - 1 - c) - 3 : oz * T + c;          // source cell of the group's lowest address
      if (lowest >= 0 && lowest + 3 < (long)g.Z * T) {
        const unsigned* p = xp + sy * g.st_y + lowest;
        const u32x4 w = load4(p, is_aligned16(p));
        u32x4 v = fz ? u32x4{w[3], w[2], w[1], w[0]} : w;
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = tone.shade(v[m]);
        return v;
      }
    }
    u32x4 v;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int cc = c + m, k = T > 1 ? cc / T : cc;
      v[m] = cell(g, j, k, cc - k * T);
    }
    return v;
  }
};

// CutMix takes a cell from one side or the other: the side is SELECTED field by field and fetched through one code path, so that lanes
// inside and outside the box do not run two fetches one after the other.  (The order of the selects, like the member-by-member writes of
// `tone` in init, is part of how the kernel is scheduled: profiles/augment_shared_layer.txt.)
__device__ __forceinline__ Side pick(bool partner, const Side& own, const Side& other) {
  Side s;
  s.xp = partner ? other.xp : own.xp;
  s.oy = partner ? other.oy : own.oy; s.oz = partner ? other.oz : own.oz;
  s.fy = partner ? other.fy : own.fy; s.fz = partner ? other.fz : own.fz;
  s.plane_in = partner ? other.plane_in : own.plane_in; s.tone.copy = partner ? other.tone.copy : own.tone.copy; s.run = partner ? other.run : own.run;
  s.tone.scale = partner ? other.tone.scale : own.tone.scale; s.tone.shift = partner ? other.tone.shift : own.tone.shift;
  s.fill = own.fill;
  return s;
}

// One workgroup of the grid (B Sx, ceil(Sy Sz T / PASS_SPAN)).  Mix = false is the apply pass: it reads no mix table and has one Side;
// everything about a partner, the blend and the box exists for Mix = true alone.
template <bool Mix>
__device__ __forceinline__ void augment_pass(const unsigned* __restrict__ src, const PassGeom& g, const int* __restrict__ aug, const int* __restrict__ mix,
                                             unsigned fill, unsigned* __restrict__ out) {
  const int tid = threadIdx.x;
  const int plane = blockIdx.x, b = plane / g.Sx, i = plane - b * g.Sx;
  const int T = g.T, L = g.Sz * T, P = g.Sy * L;           // cells of one output row (j) and of the plane
  const int e0 = blockIdx.y * PASS_SPAN, len = min(PASS_SPAN, P - e0);
  int mode = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0, partner = b;
  float lam = 1.0f;
  if constexpr (Mix) {
    const int* mrow = mix + (long)NV_MIX_COLS * b;
    partner = mrow[0];
    lam = __int_as_float(mrow[2]);
    mode = mrow[1];
    if (mode < 0 || mode > 2 || lam == 1.0f || partner < 0 || partner >= g.B) mode = 0;        // A_b alone: the partner is not read
    y0 = mrow[7]; y1 = mrow[8]; z0 = mrow[9]; z1 = mrow[10];
    const bool x_in = i >= mrow[5] && i < mrow[6];         // (cutmix) this plane crosses the box
    if (mode == 2 && !x_in) mode = 0;
  }
  const float mu = 1.0f - lam;
  Side own, other;                                         // (other: the partner under its own row, Mix alone)
  own.init(src, g, aug, b, i, fill);
  if constexpr (Mix) other.init(src, g, aug, mode ? partner : b, i, fill);
  const long first = (long)plane * P + e0;
  unsigned* o = out + first;
  const Span s = split_span(first, len);
  if (!Mix && !own.plane_in) {                             // (uniform over the workgroup) the whole plane lies outside the volume
    const u32x4 fill4 = {fill, fill, fill, fill};
    for (int e = tid; e < s.head; e += PASS_THREADS) o[e] = fill;
    for (int e = s.tail + tid; e < len; e += PASS_THREADS) o[e] = fill;
    for (int q = tid; q < s.groups; q += PASS_THREADS) *reinterpret_cast<u32x4*>(o + s.head + 4 * q) = fill4;
    return;
  }
  auto blend = [&](unsigned a, unsigned p) {
    const float l = lam * __uint_as_float(a), r = mu * __uint_as_float(p);
    return __float_as_uint(l + r);
  };
  auto single = [&](int e) {
    const int j = (e0 + e) / L, c = (e0 + e) - j * L, k = T > 1 ? c / T : c, t = c - k * T;
    if (!Mix || mode == 0) return own.cell(g, j, k, t);
    if (mode == 1) return blend(own.cell(g, j, k, t), other.cell(g, j, k, t));
    return pick(j >= y0 && j < y1 && k >= z0 && k < z1, own, other).cell(g, j, k, t);
  };
  for (int e = tid; e < s.head; e += PASS_THREADS) o[e] = single(e);
  for (int e = s.tail + tid; e < len; e += PASS_THREADS) o[e] = single(e);
  for (int q = tid; q < s.groups; q += PASS_THREADS) {
    const int e = s.head + 4 * q;
    const int j = (e0 + e) / L, c = (e0 + e) - j * L;
    u32x4 v;
    if (c + 3 < L) {                                       // the four cells share the output row j
      if (!Mix || mode == 0) {
        v = own.group(g, j, c);
      } else if (mode == 1) {
        const u32x4 a = own.group(g, j, c), p = other.group(g, j, c);
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = blend(a[m], p[m]);
      } else if (j < y0 || j >= y1) {
        v = own.group(g, j, c);
      } else {
        // a row that crosses the box: both sides' groups are fetched side by side - unless the group lies wholly outside (inside) the
        // box in z, then only the sample's (the partner's) - and every cell takes its side.  No cell-by-cell path for a group that a z
        // face cuts: nearly every wave of such a row holds one, and would wait for it.
        const int k_lo = T > 1 ? c / T : c, k_hi = T > 1 ? (c + 3) / T : c + 3;
        const bool none_in = k_hi < z0 || k_lo >= z1, all_in = k_lo >= z0 && k_hi < z1;
        u32x4 a = {0, 0, 0, 0}, p = {0, 0, 0, 0};
        if (!all_in) a = own.group(g, j, c);
        if (!none_in) p = other.group(g, j, c);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int k = T > 1 ? (c + m) / T : c + m;
          v[m] = (k >= z0 && k < z1) ? p[m] : a[m];
        }
      }
    } else {                                               // the group straddles output rows (e + m < len: every cell lies in the plane)
#pragma unroll
      for (int m = 0; m < 4; ++m) v[m] = single(e + m);
    }
    *reinterpret_cast<u32x4*>(o + e) = v;
  }
}

__global__ __launch_bounds__(PASS_THREADS) void augment_apply_kernel(const unsigned* __restrict__ src, PassGeom g, const int* __restrict__ params, unsigned fill,
                                                                     unsigned* __restrict__ out) {
  augment_pass<false>(src, g, params, nullptr, fill, out);
}
__global__ __launch_bounds__(PASS_THREADS) void augment_mix_kernel(const unsigned* __restrict__ src, PassGeom g, const int* __restrict__ aug, const int* __restrict__ mix,
                                                                   unsigned fill, unsigned* __restrict__ out) {
  augment_pass<true>(src, g, aug, mix, fill, out);
}
}  // namespace

extern "C" int nv_augment_params(const nv_augment_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* params, void* stream) {
  NV_CHECK_ARG(cfg && params && B > 0 && rank >= 0, "nv_augment_params: bad arguments (null pointer, B not positive or a negative rank)");
  NV_CHECK_ARG(cfg->struct_size == (int)sizeof(nv_augment_config), "nv_augment_params: struct_size %d, this library's nv_augment_config has %d bytes",
               cfg->struct_size, (int)sizeof(nv_augment_config));
  NV_CHECK_ARG(nv_aligned(params, 4), "nv_augment_params: params 4-byte aligned");
  AugDraw d;
  if (const int rc = window_draw_setup("nv_augment_params", *cfg, d)) return rc;
  for (int a = 0; a < 3; ++a) {
    const int m = cfg->max_shift[a];
    NV_CHECK_ARG(m >= 0 && m < (1 << 30), "nv_augment_params: axis %d: max_shift %d outside [0, 2^30)", a, m);
    d.max_shift[a] = m;
  }
  hipLaunchKernelGGL(augment_params_kernel, dim3((B + PASS_THREADS - 1) / PASS_THREADS), dim3(PASS_THREADS), 0, (hipStream_t)stream, d, (uint64_t)seed,
                     (uint64_t)step, (uint64_t)rank, B, params);
  NV_CHECK_LAUNCH("nv_augment_params");
  return NV_OK;
}

extern "C" int nv_augment_apply(const float* src, const long* strides5, int B, const int* in3, int T, const int* params, const int* roi3, float fill,
                                float* out, void* stream) {
  const char* who = "nv_augment_apply";
  PassLaunch l;
  if (const int rc = pass_setup(who, "params", src, strides5, B, in3, T, params, nullptr, roi3, fill, out, l)) return rc;
  hipLaunchKernelGGL(augment_apply_kernel, l.grid, dim3(PASS_THREADS), 0, (hipStream_t)stream, (const unsigned*)src, l.g, params, l.fill, (unsigned*)out);
  NV_CHECK_LAUNCH(who);
  return NV_OK;
}

extern "C" int nv_augment_mix(const float* src, const long* strides5, int B, const int* in3, int T, const int* aug, const int* mix, const int* roi3, float fill,
                              float* out, void* stream) {
  const char* who = "nv_augment_mix";
  PassLaunch l;                            // (the augmentation rows may be missing: identity rows)
  if (const int rc = pass_setup(who, "the two tables", src, strides5, B, in3, T, mix, aug, roi3, fill, out, l)) return rc;
  hipLaunchKernelGGL(augment_mix_kernel, l.grid, dim3(PASS_THREADS), 0, (hipStream_t)stream, (const unsigned*)src, l.g, aug, mix, l.fill, (unsigned*)out);
  NV_CHECK_LAUNCH(who);
  return NV_OK;
}
