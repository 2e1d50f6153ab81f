// Random affine augmentation on the device (neurovit_amd.augment.VolumeAffine): per sample a rotation about the centre of the window, a zoom
// and a sub-voxel translation on top of the crop, flips and intensity change of VolumeAugment, for 3D volumes and 4D series - one streaming
// GATHER pass with trilinear interpolation.  It is the one kernel of this library whose reads are not index copies.
//
//   nv_affine_params   (config, seed, step, rank) -> table int32 [B, 16]: the fp32 bit patterns of the 3 x 4 map output cell -> source
//                      coordinate (12), bits of scale and shift, flags, 0 - drawn and formed in double on the device, rounded to fp32 once
//                      (the rule is in the header; tests/affine_ref.py restates it)
//   nv_affine_apply    src fp32 [B, X, Y, Z, T] (any strides) + table -> out fp32 [B, Sx, Sy, Sz, T] dense
//
// The work split is that of augment.hip: a workgroup owns PASS_SPAN consecutive elements of one output plane (b, i), stores go out in 16-byte
// groups at any alignment of the plane (split_span), and the coordinates of every cell are formed from its indices (never incrementally).
// Corners are fetched straight through the vector cache - under the small rotations of real use neighbouring cells share most of
// theirs - and all of a thread's corners before it looks at any: the fetch is free of branches, so the loads overlap.  Three paths:
//   a resampled volume   lane l of a wave computes cells l, l + 64, l + 128, l + 192 of the wave's 256, so that one load instruction reads
//                        neighbours of a source row; the wave turns them into 16-byte groups through its kilobyte of LDS
//   a resampled series   a group that lies within one voxel (every group when T is a multiple of four) does the coordinate work once
//                        and reads each corner as a run of four timepoints
//   an integer row       all twelve numbers integers (an unapplied sample, a hand-written crop / flip / quarter turn): no fractions, one
//                        load per cell, and one 16-byte load per group where four cells of an output row are four neighbours of a
//                        source row that is contiguous in memory
//
// The arithmetic is fp32, every operation rounded on its own (contraction is off for the whole file), in the order the header spells out;
// voxels move as 32-bit patterns wherever no arithmetic touches them.  The range tests happen on the float coordinate BEFORE it is
// converted: no index is formed from a NaN, an infinity or a value outside [-1, N).  No atomics, every output element is written once.
// The draw rule, the intensity change, the geometry and the host-side checks are those of augment.hip: augment_common.h.
#include "augment_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int AF_COLS = 16;
constexpr int AF_MAX_DIM = 1 << 24;      // every index of the volume is exact in fp32

// ------------------------------------------------------------------------------------------------ parameters
struct AffDraw {
  unsigned crop_n[3];                    // X - Sx + 1: the crop offset is uniform on [0, crop_n)
  double half[3];                        // (S - 1) / 2: the centre of the window
  double rotate_deg[3], zoom_lo, zoom_hi, translate[3];
  int isotropic;
  unsigned prob_thresh, flip_thresh[3];  // (unsigned)(p * 65536)
  float scale_lo, scale_hi, shift_lo, shift_hi;
};

__device__ __forceinline__ double aff_real(uint64_t h) { return (double)(h >> 11) * 0x1p-53; }         // 53 bits: exact

// c = a b, every sum from the left
__device__ __forceinline__ void mat3(const double (&a)[3][3], const double (&b)[3][3], double (&c)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) c[r][q] = (a[r][0] * b[0][q] + a[r][1] * b[1][q]) + a[r][2] * b[2][q];
}

// One thread per sample: draw d of sample b at step s hashes the counter ((s 2^32 + b) 32 + d) mod 2^64 in the affine domain of the rank's seed.
__global__ __launch_bounds__(PASS_THREADS) void affine_params_kernel(AffDraw cfg, uint64_t seed, uint64_t step, uint64_t rank, int B, int* __restrict__ table) {
  const int b = blockIdx.x * PASS_THREADS + threadIdx.x;
  if (b >= B) return;
  const SampleDraws h(seed, rank, AFFINE_DOMAIN, AFFINE_STRIDE, step, b);
  int flags = 0;
  double o[3], f[3], theta[3] = {0.0, 0.0, 0.0}, zoom[3] = {1.0, 1.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = (double)draw_below(h(a), cfg.crop_n[a]);
    const bool flip = draw_chance(h(3 + a), cfg.flip_thresh[a]);
    if (flip) flags |= 1 << a;
    f[a] = flip ? -1.0 : 1.0;
  }
  const bool applied = draw_chance(h(6), cfg.prob_thresh);
  double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (applied) {
    flags |= 8;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      theta[a] = (2.0 * aff_real(h(7 + a)) - 1.0) * cfg.rotate_deg[a] * (3.141592653589793 / 180.0);
      zoom[a] = cfg.zoom_lo + (cfg.zoom_hi - cfg.zoom_lo) * aff_real(h(cfg.isotropic ? 10 : 10 + a));
      t[a] = (2.0 * aff_real(h(13 + a)) - 1.0) * cfg.translate[a];
    }
    const double cx = cos(theta[0]), sx = sin(theta[0]), cy = cos(theta[1]), sy = sin(theta[1]), cz = cos(theta[2]), sz = sin(theta[2]);
    const double Rx[3][3] = {{1.0, 0.0, 0.0}, {0.0, cx, -sx}, {0.0, sx, cx}};
    const double Ry[3][3] = {{cy, 0.0, sy}, {0.0, 1.0, 0.0}, {-sy, 0.0, cy}};
    const double Rz[3][3] = {{cz, -sz, 0.0}, {sz, cz, 0.0}, {0.0, 0.0, 1.0}};
    double Ryx[3][3];
    mat3(Ry, Rx, Ryx);
    mat3(Rz, Ryx, R);
  }
  int row[AF_COLS];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double M[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) M[q] = R[a][q] * (f[q] / zoom[q]);
    const double through = (M[0] * cfg.half[0] + M[1] * cfg.half[1]) + M[2] * cfg.half[2];
    const double m3 = ((o[a] + t[a]) + cfg.half[a]) - through;
#pragma unroll
    for (int q = 0; q < 3; ++q) row[4 * a + q] = __float_as_int((float)(M[q] + 0.0));       // (+ 0.0: a zero is +0.0)
    row[4 * a + 3] = __float_as_int((float)(m3 + 0.0));
  }
  row[12] = __float_as_int(draw_between(h(16), cfg.scale_lo, cfg.scale_hi));
  row[13] = __float_as_int(draw_between(h(17), cfg.shift_lo, cfg.shift_hi));
  row[14] = flags;
  row[15] = 0;
#pragma unroll
  for (int i = 0; i < AF_COLS; ++i) table[(long)AF_COLS * b + i] = row[i];
}

// ------------------------------------------------------------------------------------------------ the pass
// A sample's row: the map, the intensity change, and whether all twelve numbers are integers (then no cell has a fraction)
struct AffRow {
  float m[12];
  Intensity tone;
  bool integer;

  __device__ __forceinline__ void init(const int* table, int b) {
    const int* row = table + (long)AF_COLS * b;
    integer = true;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      m[q] = __int_as_float(row[q]);
      integer = integer && fabsf(m[q]) <= 16777216.0f && m[q] == floorf(m[q]);
    }
    tone.scale = __int_as_float(row[12]); tone.shift = __int_as_float(row[13]);
    tone.settle();
  }
  // the source coordinate along the axis of m[4 a ..] of output cell (i, j, k)
  __device__ __forceinline__ float coord(int a, int i, int j, int k) const {
    const float pi = m[4 * a] * (float)i, pj = m[4 * a + 1] * (float)j, pk = m[4 * a + 2] * (float)k;
    const float ij = pi + pj;
    const float ijk = ij + pk;
    return ijk + m[4 * a + 3];
  }
};

// One axis of one cell: the lower corner `lo` (in [-1, N - 1] whatever the coordinate was), which of the two corners lie inside the
// volume, the fraction, and whether the upper corner is used at all (w != 0).  Integer: the row has no fractions.
struct AffAxis {
  int lo;
  bool in_lo, in_hi, use_hi;
  float w;
};
template <bool Integer>
__device__ __forceinline__ AffAxis axis_of(float s, int N) {
  const float fl = floorf(s);
  const bool ok = s >= -1.0f && s < (float)N;              // in float, before any conversion; false for a NaN
  AffAxis a;
  a.lo = (int)(ok ? fl : -1.0f);
  a.w = Integer ? 0.0f : s - fl;
  a.use_hi = !Integer && a.w != 0.0f;
  a.in_lo = ok && a.lo >= 0;
  a.in_hi = ok && a.lo + 1 < N;
  return a;
}

__device__ __forceinline__ unsigned lerp_bits(unsigned a, unsigned b, float w) {
  const float fa = __uint_as_float(a), d = __uint_as_float(b) - fa;
  const float part = d * w;
  return __float_as_uint(fa + part);
}

// N = 1: output cell (i, j, k, t0); N = 4: the timepoints t0 .. t0 + 3 of voxel (i, j, k), which share the coordinates.  sb: the sample.
// Branch-free: every corner is fetched first, from an address CLAMPED into the volume, and what lies outside or is not used is then
// replaced by a select - so the loads of a thread's four cells are all in flight together instead of each waiting behind a branch
// (a gather is bound by the latency of its loads long before it is bound by their bytes).  An integer row has one corner per cell.
template <int N, bool Integer>
__device__ __forceinline__ void sample(const unsigned* __restrict__ sb, const PassGeom& g, const AffRow& r, int i, int j, int k, int t0, unsigned fill,
                                       bool run16, unsigned (&v)[N]) {
  constexpr int U = Integer ? 1 : 2;                       // corners per axis
  const AffAxis ax = axis_of<Integer>(r.coord(0, i, j, k), g.X), ay = axis_of<Integer>(r.coord(1, i, j, k), g.Y), az = axis_of<Integer>(r.coord(2, i, j, k), g.Z);
  // every corner this cell uses lies outside: the fill, verbatim
  const bool any_in = (ax.in_lo || (ax.use_hi && ax.in_hi)) && (ay.in_lo || (ay.use_hi && ay.in_hi)) && (az.in_lo || (az.use_hi && az.in_hi));
  const long ot = (long)t0 * g.st_t;
  const long xo[2] = {max(ax.lo, 0) * g.st_x, min(ax.lo + 1, g.X - 1) * g.st_x};
  const long yo[2] = {max(ay.lo, 0) * g.st_y, min(ay.lo + 1, g.Y - 1) * g.st_y};
  const long zo[2] = {max(az.lo, 0) * g.st_z + ot, min(az.lo + 1, g.Z - 1) * g.st_z + ot};
  const bool xin[2] = {ax.in_lo, ax.in_hi}, yin[2] = {ay.in_lo, ay.in_hi}, zin[2] = {az.in_lo, az.in_hi};
  unsigned c[U][U][U][N];
#pragma unroll
  for (int dx = 0; dx < U; ++dx)
#pragma unroll
    for (int dy = 0; dy < U; ++dy)
#pragma unroll
      for (int dz = 0; dz < U; ++dz) {
        const unsigned* p = sb + xo[dx] + yo[dy] + zo[dz];
        if constexpr (N == 4) {
          if (run16) {                                     // (uniform) the four timepoints are one aligned run of memory
            const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
            for (int n = 0; n < 4; ++n) c[dx][dy][dz][n] = q[n];
          } else {
#pragma unroll
            for (int n = 0; n < 4; ++n) c[dx][dy][dz][n] = p[n * g.st_t];
          }
        } else {
          c[dx][dy][dz][0] = *p;
        }
      }
#pragma unroll
  for (int dx = 0; dx < U; ++dx)
#pragma unroll
    for (int dy = 0; dy < U; ++dy)
#pragma unroll
      for (int dz = 0; dz < U; ++dz) {
        const bool in = xin[dx] && yin[dy] && zin[dz];
#pragma unroll
        for (int n = 0; n < N; ++n) c[dx][dy][dz][n] = in ? c[dx][dy][dz][n] : fill;
      }
  if constexpr (!Integer) {                                // along z, then y, then x; w == 0 keeps the lower corner verbatim
#pragma unroll
    for (int n = 0; n < N; ++n) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) c[dx][dy][0][n] = az.use_hi ? lerp_bits(c[dx][dy][0][n], c[dx][dy][1][n], az.w) : c[dx][dy][0][n];
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) c[dx][0][0][n] = ay.use_hi ? lerp_bits(c[dx][0][0][n], c[dx][1][0][n], ay.w) : c[dx][0][0][n];
      c[0][0][0][n] = ax.use_hi ? lerp_bits(c[0][0][0][n], c[1][0][0][n], ax.w) : c[0][0][0][n];
    }
  }
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = any_in ? r.tone.shade(c[0][0][0][n]) : fill;
}

// One workgroup of the grid (B Sx, ceil(Sy Sz T / PASS_SPAN)) under its sample's row
template <bool Integer>
__device__ __forceinline__ void affine_pass(const unsigned* __restrict__ src, const PassGeom& g, const AffRow& r, int b, int i, unsigned fill,
                                            unsigned* __restrict__ out, unsigned* tile) {
  const int tid = threadIdx.x;
  const int T = g.T, L = g.Sz * T, P = g.Sy * L;           // cells of one output row (j) and of the plane
  const int e0 = blockIdx.y * PASS_SPAN, len = min(PASS_SPAN, P - e0);
  const long first = (long)blockIdx.x * P + e0;
  unsigned* o = out + first;
  const Span s = split_span(first, len);
  const unsigned* sb = src + (long)b * g.st_b;
  // (integer rows of a volume) k moves along z alone, by one source cell, and a source row is a run of memory: four cells, one load
  const bool z_run = Integer && T == 1 && g.st_z == 1 && r.m[2] == 0.0f && r.m[6] == 0.0f && r.m[8] == 0.0f && r.m[9] == 0.0f && fabsf(r.m[10]) == 1.0f;
  // (series) time is innermost and dense, T and every stride are multiples of four and the sample starts a 16-byte group: then every
  // plane and span starts one too (head = 0), every group is the timepoints 4 n .. 4 n + 3 of one voxel, and each corner of it is
  // one aligned 16-byte load
  const bool run16 = g.st_t == 1 && (T & 3) == 0 && ((g.st_x | g.st_y | g.st_z) & 3) == 0 && is_aligned16(sb);
  auto single = [&](int e) {
    const int j = (e0 + e) / L, c = (e0 + e) - j * L, k = T > 1 ? c / T : c;
    unsigned v[1];
    sample<1, Integer>(sb, g, r, i, j, k, c - k * T, fill, false, v);
    return v[0];
  };
  for (int e = tid; e < s.head; e += PASS_THREADS) o[e] = single(e);
  for (int e = s.tail + tid; e < len; e += PASS_THREADS) o[e] = single(e);
  if (!Integer && T == 1) {
    // A resampled volume.  Four consecutive cells per lane would make every corner load of a wave a 16-byte-strided gather over a
    // kilobyte of each source row; instead lane l of a wave fetches cells l, l + 64, l + 128, l + 192 of the wave's 256 - neighbours in
    // the source row for neighbouring lanes - and the wave turns them into 16-byte groups through its kilobyte of LDS.  The trip
    // count is uniform; a cell past the end is computed as the last one (no branch in front of the loads) and not stored.
    const int wave = tid >> 6, lane = tid & 63;
    unsigned* wt = tile + 256 * wave;
    for (int q0 = 0; q0 < s.groups; q0 += PASS_THREADS) {
      const int eb = s.head + 4 * (q0 + 64 * wave);        // the wave's first cell
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int e = e0 + min(eb + lane + 64 * m, s.tail - 1);
        const int j = e / L;
        unsigned w[1];
        sample<1, false>(sb, g, r, i, j, e - j * L, 0, fill, false, w);
        wt[lane + 64 * m] = w[0];
      }
      __syncthreads();
      if (eb + 4 * lane < s.tail) *reinterpret_cast<u32x4*>(o + eb + 4 * lane) = *reinterpret_cast<const u32x4*>(wt + 4 * lane);
      __syncthreads();
    }
    return;
  }
  for (int q = tid; q < s.groups; q += PASS_THREADS) {
    const int e = s.head + 4 * q;
    const int j = (e0 + e) / L, c = (e0 + e) - j * L;
    u32x4 v;
    bool done = false;
    if (c + 3 < L) {                                       // the four cells share the output row j
      if (T > 1) {
        const int k = c / T, t = c - k * T;
        if (t + 3 < T) {                                   // ... and the voxel: its corners are runs of four timepoints
          unsigned w[4];
          sample<4, Integer>(sb, g, r, i, j, k, t, fill, run16, w);
          v = u32x4{w[0], w[1], w[2], w[3]};
          done = true;
        }
      } else if (z_run) {
        const AffAxis ax = axis_of<true>(r.coord(0, i, j, c), g.X), ay = axis_of<true>(r.coord(1, i, j, c), g.Y);
        const AffAxis z0 = axis_of<true>(r.coord(2, i, j, c), g.Z), z3 = axis_of<true>(r.coord(2, i, j, c + 3), g.Z);
        const int dz = z3.lo - z0.lo;
        if (ax.in_lo && ay.in_lo && z0.in_lo && z3.in_lo && (dz == 3 || dz == -3)) {
          const unsigned* p = sb + ax.lo * g.st_x + ay.lo * g.st_y + min(z0.lo, z3.lo);
          const u32x4 w = load4(p, is_aligned16(p));
          v = dz < 0 ? u32x4{w[3], w[2], w[1], w[0]} : w;
#pragma unroll
          for (int m = 0; m < 4; ++m) v[m] = r.tone.shade(v[m]);
          done = true;
        }
      }
    }
    if (!done) {                                           // cell by cell (e + m < len: every cell lies in the plane)
#pragma unroll
      for (int m = 0; m < 4; ++m) v[m] = single(e + m);
    }
    *reinterpret_cast<u32x4*>(o + e) = v;
  }
}

__global__ __launch_bounds__(PASS_THREADS) void affine_apply_kernel(const unsigned* __restrict__ src, PassGeom g, const int* __restrict__ table, unsigned fill,
                                                                    unsigned* __restrict__ out) {
  const int b = blockIdx.x / g.Sx, i = blockIdx.x - b * g.Sx;
  __shared__ __attribute__((aligned(16))) unsigned tile[4 * PASS_THREADS];      // a resampled volume's groups on their way from cell order to store order
  AffRow r;
  r.init(table, b);
  if (r.integer) affine_pass<true>(src, g, r, b, i, fill, out, tile);      // (uniform over the workgroup)
  else affine_pass<false>(src, g, r, b, i, fill, out, tile);
}

}  // namespace

extern "C" int nv_affine_params(const nv_affine_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* table, void* stream) {
  NV_CHECK_ARG(cfg && table && B > 0 && rank >= 0, "nv_affine_params: bad arguments (null pointer, B not positive or a negative rank)");
  NV_CHECK_ARG(cfg->struct_size == (int)sizeof(nv_affine_config), "nv_affine_params: struct_size %d, this library's nv_affine_config has %d bytes",
               cfg->struct_size, (int)sizeof(nv_affine_config));
  NV_CHECK_ARG(nv_aligned(table, 4), "nv_affine_params: table 4-byte aligned");
  AffDraw d;
  if (const int rc = window_draw_setup("nv_affine_params", *cfg, d)) return rc;
  for (int a = 0; a < 3; ++a) {
    const int X = cfg->in_size[a];
    const double deg = cfg->rotate_deg[a], tr = cfg->translate[a];
    NV_CHECK_ARG(X <= AF_MAX_DIM, "nv_affine_params: axis %d: input %d beyond 2^24", a, X);
    NV_CHECK_ARG(deg >= -180.0 && deg <= 180.0, "nv_affine_params: axis %d: rotate_deg %g outside [-180, 180]", a, deg);
    NV_CHECK_ARG(isfinite(tr) && tr >= 0.0, "nv_affine_params: axis %d: translate %g must be finite and not negative", a, tr);
    d.half[a] = (double)(cfg->roi[a] - 1) / 2.0;
    d.rotate_deg[a] = deg;
    d.translate[a] = tr;
  }
  NV_CHECK_ARG(cfg->zoom_lo > 0.0 && cfg->zoom_lo <= cfg->zoom_hi && cfg->zoom_hi <= 16.0, "nv_affine_params: zoom [%g, %g] must satisfy 0 < lo <= hi <= 16",
               cfg->zoom_lo, cfg->zoom_hi);
  NV_CHECK_ARG(cfg->prob >= 0.0 && cfg->prob <= 1.0, "nv_affine_params: prob %g outside [0, 1]", cfg->prob);
  d.zoom_lo = cfg->zoom_lo; d.zoom_hi = cfg->zoom_hi;
  d.isotropic = cfg->isotropic != 0;
  d.prob_thresh = chance_thresh(cfg->prob);
  hipLaunchKernelGGL(affine_params_kernel, dim3((B + PASS_THREADS - 1) / PASS_THREADS), dim3(PASS_THREADS), 0, (hipStream_t)stream, d, (uint64_t)seed,
                     (uint64_t)step, (uint64_t)rank, B, table);
  NV_CHECK_LAUNCH("nv_affine_params");
  return NV_OK;
}

extern "C" int nv_affine_apply(const float* src, const long* strides5, int B, const int* in3, int T, const int* table, const int* roi3, float fill,
                               float* out, void* stream) {
  const char* who = "nv_affine_apply";
  PassLaunch l;
  if (const int rc = pass_setup(who, "table", src, strides5, B, in3, T, table, nullptr, roi3, fill, out, l)) return rc;
  const PassGeom& g = l.g;
  NV_CHECK_ARG(g.X <= AF_MAX_DIM && g.Y <= AF_MAX_DIM && g.Z <= AF_MAX_DIM, "%s: input %d x %d x %d beyond 2^24 cells along an axis", who, g.X, g.Y, g.Z);
  // the elements of src that the strides can reach against the dense output: a gather that overwrote its own source would race
  long lowest = 0, highest = 0;
  const long extent[5] = {B, g.X, g.Y, g.Z, T};
  for (int a = 0; a < 5; ++a) {
    const long reach = (extent[a] - 1) * strides5[a];
    if (reach < 0) lowest += reach; else highest += reach;
  }
  const float* out_end = out + (long)B * g.Sx * g.Sy * g.Sz * T;
  NV_CHECK_ARG(out_end <= src + lowest || src + highest < out, "%s: out aliases src", who);
  hipLaunchKernelGGL(affine_apply_kernel, l.grid, dim3(PASS_THREADS), 0, (hipStream_t)stream, (const unsigned*)src, g, table, l.fill, (unsigned*)out);
  NV_CHECK_LAUNCH(who);
  return NV_OK;
}
