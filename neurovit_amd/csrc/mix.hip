// Mixup / CutMix on the device (neurovit_amd.augment.VolumeMix), for 3D volumes and 4D series: the second half of the training
// augmentation, fused with the first so that a batch is still read once and written once.
//
//   nv_mix_params    (config, seed, step, rank) -> mix int32 [B, NV_MIX_COLS]: {partner, mode, bits of the pixel lambda, bits of the label
//                    lambda, tries, x0, x1, y0, y1, z0, z1, 0}, drawn on the device with nv_hash64 in a domain of its own (the rule is in
//                    the header; tests/mix_ref.py restates it).  lambda ~ Beta(alpha, alpha) by Joehnk's rule in double; the CutMix box in fp32.
//   nv_augment_mix   src fp32 [B, X, Y, Z, T] (any strides) + augmentation rows (or none) + mix rows -> out fp32 [B, Sx, Sy, Sz, T] dense:
//                    out = A_b, (lambda A_b) + (mu A_p), or A_p inside the box and A_b outside, where A_s is what nv_augment_apply writes
//                    for sample s under its OWN row.
//
// The pass is laid out like nv_augment_apply (augment.hip): a workgroup owns MX_SPAN consecutive elements of one output plane (b, i), the
// 16-byte groups follow the alignment of the plane in `out` (split_span), a group whose four cells lie in one source row that is a run of
// memory is read with one 16-byte load, everything else is gathered cell by cell.  A sample and its partner have rows of their own, so
// each side decides on its own whether a group is one load.  A CutMix group in a row outside the box is the sample's own; in a row that
// crosses the box both sides' groups are fetched and every cell takes its side (x and y are uniform over a group, z is not).  Voxels
// move as 32-bit patterns; the intensity change and the Mixup blend are separately rounded operations (contraction is off for the whole
// file).  No atomics, every output element is written once by one thread.
#include "attr_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int MX_THREADS = 256;
constexpr int MX_SPAN = 4096;            // elements of one output plane a workgroup owns: four 16-byte groups per thread
constexpr int MX_TRIES = 64;

// ------------------------------------------------------------------------------------------------ parameters
struct MixDraw {
  int S[3];
  double inv_alpha_mixup, inv_alpha_cutmix;      // 0 = that mode is off
  unsigned prob_thresh, switch_thresh;           // (unsigned)(p * 65536)
};

__device__ __forceinline__ double unit_open(uint64_t h) { return ((double)(h >> 12) + 0.5) * 0x1p-52; }   // 52 bits + a half: exact, never 0

// One thread per sample: draw d of sample b at step s hashes the counter ((s 2^32 + b) 256 + d) mod 2^64 under the rank's mix seed.
__global__ __launch_bounds__(MX_THREADS) void mix_params_kernel(MixDraw cfg, uint64_t seed, uint64_t step, uint64_t rank, int B, int* __restrict__ mix) {
  const int b = blockIdx.x * MX_THREADS + threadIdx.x;
  if (b >= B) return;
  const uint64_t seed_m = nv_hash64(nv_hash64(seed, rank), 0x4D4958ull);
  const uint64_t counter = ((step << 32) + (uint64_t)b) * 256u;
  auto h = [&](unsigned d) { return nv_hash64(seed_m, counter + d); };
  const int partner = B - 1 - b;
  int row[NV_MIX_COLS] = {partner, 0, __float_as_int(1.0f), __float_as_int(1.0f), 0, 0, 0, 0, 0, 0, 0, 0};
  int mode = 0;
  if (partner != b && (unsigned)(h(0) >> 48) < cfg.prob_thresh) {
    const bool mixup = cfg.inv_alpha_mixup != 0.0, cutmix = cfg.inv_alpha_cutmix != 0.0;
    if (mixup && cutmix) mode = (unsigned)(h(1) >> 48) < cfg.switch_thresh ? 2 : 1;
    else mode = cutmix ? 2 : (mixup ? 1 : 0);
  }
  if (mode) {
    const double inv_alpha = mode == 2 ? cfg.inv_alpha_cutmix : cfg.inv_alpha_mixup;
    double x = 0.0, y = 0.0;
    int t = 0;
    for (; t < MX_TRIES; ++t) {                                   // Joehnk: accept the first pair with x + y <= 1
      x = pow(unit_open(h(16 + 2 * t)), inv_alpha);
      y = pow(unit_open(h(17 + 2 * t)), inv_alpha);
      if (x + y <= 1.0) break;
    }
    const float lam = (float)(x / (x + y));
    row[1] = mode;
    row[2] = __float_as_int(lam);
    row[3] = row[2];
    row[4] = t < MX_TRIES ? t + 1 : MX_TRIES;
    if (mode == 2) {
      const float r = __fsqrt_rn(1.0f - lam);
      long cells = 1;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int S = cfg.S[a];
        const int e = (int)((float)S * r);
        const int c = (int)(((h(2 + a) >> 32) * (uint64_t)S) >> 32);
        const int lo = max(c - e / 2, 0), hi = min(c + e / 2, S);
        row[5 + 2 * a] = lo;
        row[6 + 2 * a] = hi;
        cells *= hi - lo;
      }
      const double total = (double)cfg.S[0] * (double)cfg.S[1] * (double)cfg.S[2];
      row[3] = __float_as_int((float)(1.0 - (double)cells / total));
    }
  }
#pragma unroll
  for (int i = 0; i < NV_MIX_COLS; ++i) mix[(long)NV_MIX_COLS * b + i] = row[i];
}

// ------------------------------------------------------------------------------------------------ the mixing pass
struct MixGeom {
  int B, X, Y, Z, T, Sx, Sy, Sz;
  long st_b, st_x, st_y, st_z, st_t;     // element strides of src
};

// What nv_augment_apply writes for one sample on output plane i: the cells of A_s, singly or four at a time.  Every read is
// bounds-checked against the volume, and a cell outside it gets `fill`.
struct Side {
  const unsigned* xp;                    // the source plane (valid when plane_in)
  long oy, oz;
  bool fy, fz, plane_in, copy, run;
  float scale, shift;
  unsigned fill;

  __device__ __forceinline__ void init(const unsigned* src, const MixGeom& g, const int* aug, int s, int i, unsigned fill_bits) {
    long ox = 0;
    int flips = 0;
    oy = 0; oz = 0; scale = 1.0f; shift = 0.0f;
    if (aug) {                                             // (a NULL table is identity rows)
      const int* row = aug + 8L * s;
      ox = row[0]; oy = row[1]; oz = row[2]; flips = row[3];
      scale = __int_as_float(row[4]); shift = __int_as_float(row[5]);
    }
    fy = flips & 2; fz = flips & 4;
    copy = scale == 1.0f && shift == 0.0f;
    fill = fill_bits;
    const long sx = ox + ((flips & 1) ? g.Sx - 1 - i : i);
    plane_in = sx >= 0 && sx < g.X;
    xp = src + (long)s * g.st_b + (plane_in ? sx : 0) * g.st_x;
    // a source row is one run of memory: ascending for a series with time innermost, in either direction for a volume
    run = g.T > 1 ? (g.st_t == 1 && g.st_z == g.T && !fz) : g.st_z == 1;
  }
  __device__ __forceinline__ unsigned shade(unsigned u) const {
    if (copy) return u;
    const float m = __uint_as_float(u) * scale;
    return __float_as_uint(m + shift);
  }
  // output cell (j, k, t) of the plane
  __device__ __forceinline__ unsigned cell(const MixGeom& g, int j, int k, int t) const {
    const long sy = oy + (fy ? g.Sy - 1 - j : j), sz = oz + (fz ? g.Sz - 1 - k : k);
    if (!plane_in || sy < 0 || sy >= g.Y || sz < 0 || sz >= g.Z) return fill;
    return shade(xp[sy * g.st_y + sz * g.st_z + t * g.st_t]);
  }
  // the four cells c .. c + 3 of output row j (c + 3 < Sz T): one 16-byte load where the source allows it
  __device__ __forceinline__ u32x4 group(const MixGeom& g, int j, int c) const {
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
        for (int m = 0; m < 4; ++m) v[m] = shade(v[m]);
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
// inside and outside the box do not run two fetches one after the other.
__device__ __forceinline__ Side pick(bool partner, const Side& own, const Side& other) {
  Side s;
  s.xp = partner ? other.xp : own.xp;
  s.oy = partner ? other.oy : own.oy; s.oz = partner ? other.oz : own.oz;
  s.fy = partner ? other.fy : own.fy; s.fz = partner ? other.fz : own.fz;
  s.plane_in = partner ? other.plane_in : own.plane_in; s.copy = partner ? other.copy : own.copy; s.run = partner ? other.run : own.run;
  s.scale = partner ? other.scale : own.scale; s.shift = partner ? other.shift : own.shift;
  s.fill = own.fill;
  return s;
}

// Grid (B Sx, ceil(Sy Sz T / MX_SPAN)).
__global__ __launch_bounds__(MX_THREADS) void augment_mix_kernel(const unsigned* __restrict__ src, MixGeom g, const int* __restrict__ aug, const int* __restrict__ mix,
                                                                 unsigned fill, unsigned* __restrict__ out) {
  const int tid = threadIdx.x;
  const int plane = blockIdx.x, b = plane / g.Sx, i = plane - b * g.Sx;
  const int T = g.T, L = g.Sz * T, P = g.Sy * L;           // cells of one output row (j) and of the plane
  const int e0 = blockIdx.y * MX_SPAN, len = min(MX_SPAN, P - e0);
  const int* mrow = mix + (long)NV_MIX_COLS * b;
  const int partner = mrow[0];
  const float lam = __int_as_float(mrow[2]);
  int mode = mrow[1];
  if (mode < 0 || mode > 2 || lam == 1.0f || partner < 0 || partner >= g.B) mode = 0;        // A_b alone: the partner is not read
  const float mu = 1.0f - lam;
  const int y0 = mrow[7], y1 = mrow[8], z0 = mrow[9], z1 = mrow[10];
  const bool x_in = i >= mrow[5] && i < mrow[6];           // (cutmix) this plane crosses the box
  if (mode == 2 && !x_in) mode = 0;
  Side own, other;
  own.init(src, g, aug, b, i, fill);
  other.init(src, g, aug, mode ? partner : b, i, fill);
  const long first = (long)plane * P + e0;
  unsigned* o = out + first;
  const Span s = split_span(first, len);
  auto blend = [&](unsigned a, unsigned p) {
    const float l = lam * __uint_as_float(a), r = mu * __uint_as_float(p);
    return __float_as_uint(l + r);
  };
  auto single = [&](int e) {
    const int j = (e0 + e) / L, c = (e0 + e) - j * L, k = T > 1 ? c / T : c, t = c - k * T;
    if (mode == 0) return own.cell(g, j, k, t);
    if (mode == 1) return blend(own.cell(g, j, k, t), other.cell(g, j, k, t));
    return pick(j >= y0 && j < y1 && k >= z0 && k < z1, own, other).cell(g, j, k, t);
  };
  for (int e = tid; e < s.head; e += MX_THREADS) o[e] = single(e);
  for (int e = s.tail + tid; e < len; e += MX_THREADS) o[e] = single(e);
  for (int q = tid; q < s.groups; q += MX_THREADS) {
    const int e = s.head + 4 * q;
    const int j = (e0 + e) / L, c = (e0 + e) - j * L;
    u32x4 v;
    if (c + 3 < L) {                                       // the four cells share the output row j
      if (mode == 0) {
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
}  // namespace

extern "C" int nv_mix_params(const nv_mix_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* mix, void* stream) {
  NV_CHECK_ARG(cfg && mix && B > 0 && rank >= 0, "nv_mix_params: bad arguments (null pointer, B not positive or a negative rank)");
  NV_CHECK_ARG(cfg->struct_size == (int)sizeof(nv_mix_config), "nv_mix_params: struct_size %d, this library's nv_mix_config has %d bytes", cfg->struct_size,
               (int)sizeof(nv_mix_config));
  NV_CHECK_ARG(nv_aligned(mix, 4), "nv_mix_params: mix 4-byte aligned");
  MixDraw d;
  for (int a = 0; a < 3; ++a) {
    NV_CHECK_ARG(cfg->roi[a] > 0, "nv_mix_params: axis %d: roi %d must be positive", a, cfg->roi[a]);
    d.S[a] = cfg->roi[a];
  }
  const double alphas[2] = {cfg->mixup_alpha, cfg->cutmix_alpha};
  for (int m = 0; m < 2; ++m)
    NV_CHECK_ARG(alphas[m] == 0.0 || (alphas[m] >= 0.05 && alphas[m] <= 1.0), "nv_mix_params: %s alpha %g outside [0.05, 1] (0 = off)", m ? "cutmix" : "mixup", alphas[m]);
  NV_CHECK_ARG(cfg->prob >= 0.0 && cfg->prob <= 1.0 && cfg->switch_prob >= 0.0 && cfg->switch_prob <= 1.0, "nv_mix_params: prob %g / switch_prob %g outside [0, 1]",
               cfg->prob, cfg->switch_prob);
  d.inv_alpha_mixup = alphas[0] != 0.0 ? 1.0 / alphas[0] : 0.0;
  d.inv_alpha_cutmix = alphas[1] != 0.0 ? 1.0 / alphas[1] : 0.0;
  d.prob_thresh = (unsigned)(cfg->prob * 65536.0);
  d.switch_thresh = (unsigned)(cfg->switch_prob * 65536.0);
  hipLaunchKernelGGL(mix_params_kernel, dim3((B + MX_THREADS - 1) / MX_THREADS), dim3(MX_THREADS), 0, (hipStream_t)stream, d, (uint64_t)seed, (uint64_t)step,
                     (uint64_t)rank, B, mix);
  NV_CHECK_LAUNCH("nv_mix_params");
  return NV_OK;
}

extern "C" int nv_augment_mix(const float* src, const long* strides5, int B, const int* in3, int T, const int* aug, const int* mix, const int* roi3, float fill,
                              float* out, void* stream) {
  NV_CHECK_ARG(src && strides5 && in3 && mix && roi3 && out && B > 0 && T > 0, "nv_augment_mix: bad arguments (null pointer, or B / T not positive)");
  MixGeom g;
  g.B = B; g.X = in3[0]; g.Y = in3[1]; g.Z = in3[2]; g.T = T; g.Sx = roi3[0]; g.Sy = roi3[1]; g.Sz = roi3[2];
  NV_CHECK_ARG(g.X > 0 && g.Y > 0 && g.Z > 0 && g.Sx > 0 && g.Sy > 0 && g.Sz > 0, "nv_augment_mix: input %d x %d x %d and roi %d x %d x %d must be positive", g.X,
               g.Y, g.Z, g.Sx, g.Sy, g.Sz);
  NV_CHECK_ARG(g.Sx <= g.X && g.Sy <= g.Y && g.Sz <= g.Z, "nv_augment_mix: roi %d x %d x %d is larger than the input %d x %d x %d", g.Sx, g.Sy, g.Sz, g.X, g.Y,
               g.Z);
  const long planes = (long)B * g.Sx, P = (long)g.Sy * g.Sz * T, spans = (P + MX_SPAN - 1) / MX_SPAN;
  NV_CHECK_ARG(planes < (1L << 31) && spans <= 65535 && (long)g.Z * T < (1L << 31),
               "nv_augment_mix: %ld output planes of %ld cells beyond one launch (at most 2^31 - 1 planes of %ld cells)", planes, P, 65535L * MX_SPAN);
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned(src, 4) && nv_aligned(aug, 4) && nv_aligned(mix, 4),
               "nv_augment_mix: out 16-byte aligned, src and the two tables 4-byte aligned");
  g.st_b = strides5[0]; g.st_x = strides5[1]; g.st_y = strides5[2]; g.st_z = strides5[3]; g.st_t = strides5[4];
  union { float f; unsigned u; } fbits;
  fbits.f = fill;
  hipLaunchKernelGGL(augment_mix_kernel, dim3((unsigned)planes, (unsigned)spans), dim3(MX_THREADS), 0, (hipStream_t)stream, (const unsigned*)src, g, aug, mix,
                     fbits.u, (unsigned*)out);
  NV_CHECK_LAUNCH("nv_augment_mix");
  return NV_OK;
}
