"""CPU checks of the random affine augmentation (no GPU): the C-ABI pieces csrc/affine.hip adds within revision 8 (nv_affine_params,
nv_affine_apply), the refusals of neurovit_amd.augment.VolumeAffine and of the Trainer keys, and the CPU restatement
(tests/affine_ref.py) that the GPU tests (tests/test_affine_gpu.py) hold the kernel to bit for bit:

  geometry       the float64 restatement against F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True) in float64, grid
                 2 s_a / (N_a - 1) - 1 in (z, y, x) order, 20 x 19 x 18 -> 16 x 17 x 16 under random rotations, anisotropic zoom, flips and
                 translations: within 1e-12 (the two write the lerp differently: a + (b - a) w against (1 - w) a + w b; a prototype
                 measured 9e-15); a non-zero fill through sample(x - fill) + fill;
  rounding       the fp32 restatement against the float64 one, per cell, within 2^-24 (4 R A + 8 V) (affine_ref.bound), at 20^3 and 40^3;
  integer maps   crops, every flip combination and offsets that leave the volume equal the index copy of tests/augment_ref.py bit for
                 bit (NaN payloads, +-inf, -0.0 planted); exact quarter turns equal torch.rot90;
  teeth          on the inputs of the GPU bit gate, a fused lerp, a lerp in x-y-z order and an incrementally advanced coordinate each
                 differ from the restatement in at least one cell;
  draws          deterministic in (seed, rank, step, b), different between ranks, independent of B; prob 0 / 1 never / always applies;
                 unapplied rows are integer maps exactly;
  refusals       every argument error of VolumeAffine, of the two entry points and of the Trainer keys that needs no device.
"""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import affine_ref as R
import augment_ref as A

NAMES = ("nv_affine_params", "nv_affine_apply")


# ------------------------------------------------------------------ symbols and ABI
def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NAMES:
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    protos = _cabi.lib.protos
    assert protos["nv_affine_params"][1] == protos["nv_augment_params"][1] and protos["nv_affine_apply"][1] == protos["nv_augment_apply"][1]
    assert _cabi.ABI_VERSION == 8 and dll.nv_abi_version() == 8          # new symbols only


def test_the_package_exports_volume_affine():
    import neurovit_amd
    from neurovit_amd.augment import VolumeAffine
    assert neurovit_amd.VolumeAffine is VolumeAffine


# ------------------------------------------------------------------ (a) geometry
def random_table(B, roi, in_size, seed, zoom=(0.8, 1.25)):
    """rotations up to 25 degrees per axis, anisotropic zoom, flips, translations up to 2.5 voxels, crop offsets in range"""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: (lo + (hi - lo) * torch.rand(3, generator=g, dtype=torch.float64)).tolist()
    maps = []
    for b in range(B):
        offset = [int(torch.randint(0, n - s + 1, (1,), generator=g)) for n, s in zip(in_size, roi)]
        maps.append(R.map_rows(roi, offset, b % 8, [math.radians(d) for d in u(-25, 25)], u(*zoom), u(-2.5, 2.5)))
    return R.table_of(maps)


def by_grid_sample(x, table, roi, fill):
    """F.grid_sample in float64 under the table's maps: grid 2 s_a / (N_a - 1) - 1 in (z, y, x) order, zero padding moved to `fill`"""
    B = x.shape[0]
    size = x.shape[1:4]
    i, j, k = (torch.arange(roi[a], dtype=torch.float64).view([-1 if q == a else 1 for q in range(3)]) for a in range(3))
    grids = []
    for b in range(B):
        m = table[b, :12].view(torch.float32).double().tolist()
        s = [(m[4 * a] * i + m[4 * a + 1] * j + m[4 * a + 2] * k + m[4 * a + 3]).expand(*roi) for a in range(3)]
        grids.append(torch.stack([2.0 * s[a] / (size[a] - 1) - 1.0 for a in (2, 1, 0)], dim=-1))
    out = F.grid_sample((x.double() - fill)[:, None], torch.stack(grids), mode="bilinear", padding_mode="zeros", align_corners=True)
    return out[:, 0] + fill


@pytest.mark.parametrize("fill", [0.0, -2.5])
def test_float64_restatement_is_grid_sample(fill):
    roi = (16, 17, 16)
    x = R.volume(B=8, seed=11)
    table = random_table(8, roi, R.IN, seed=12)
    got = R.apply_ref(x, table, roi, fill, dtype=torch.float64)
    want = by_grid_sample(x, table, roi, fill)
    err = (got - want).abs().max().item()
    print(f"float64 restatement against grid_sample, fill {fill}: max abs {err:.3e}")
    assert err < 1e-12
    assert (got != fill).float().mean() > 0.5 and (got == fill).any()            # most cells are sampled, some lie wholly outside


# ------------------------------------------------------------------ (b) rounding
@pytest.mark.parametrize("n", [20, 40])
def test_fp32_restatement_within_the_first_order_bound(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(4, n, n, n, generator=g)
    roi = (n - 4, n - 3, n - 4)
    table = random_table(4, roi, (n, n, n), seed=n + 1)
    for fill in (0.0, 1.5):
        got, exact = R.apply_ref(x, table, roi, fill), R.apply_ref(x, table, roi, fill, dtype=torch.float64)
        err, limit = (got.double() - exact).abs(), R.bound(x, table, roi, fill)
        share = (err / limit).max().item()
        print(f"fp32 against float64 restatement at {n}^3, fill {fill}: largest share of the bound {share:.3f}")
        assert (err <= limit).all()


# ------------------------------------------------------------------ (c) integer maps
def special_volume(shape, seed):
    """NaN (one with a payload), +-inf, -0.0 among normal values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(shape[0], -1)
    flat[:, 0::17] = float("nan")
    flat[:, 1::19] = float("inf")
    flat[:, 2::23] = float("-inf")
    flat[:, 3::29] = -0.0
    flat[:, 5::31] = torch.tensor([0x7fc01234], dtype=torch.int32).view(torch.float32)[0]
    return x


@pytest.mark.parametrize("T", [None, 3])
def test_integer_maps_equal_the_index_copy_bit_for_bit(T):
    shape = (1, 9, 8, 7) if T is None else (1, 9, 8, 7, T)
    x = special_volume(shape, 5)
    roi = (6, 5, 7)
    offsets = [(0, 0, 0), (3, 3, 0), (1, 2, 0), (-2, 1, 0), (2, -3, 1), (0, 0, -4), (5, 0, 0), (0, 6, 3), (-6, 0, 0), (0, 8, 0), (-40, 50, -60)]
    for offset, flips in itertools.product(offsets, range(8)):
        table = R.table_of([R.integer_map(roi, offset, flips)])
        want = A.apply_ref(x, R.augment_rows([(offset, flips)]), roi, fill=-2.5)
        got = R.apply_ref(x, table, roi, fill=-2.5)
        assert torch.equal(A.bits(got), A.bits(want)), (offset, flips)
    scale, shift = torch.tensor([0.75, -0.3]).view(torch.int32).tolist()
    plain = torch.randn(shape, generator=torch.Generator().manual_seed(6))
    for offset, flips in (((1, 2, 0), 5), ((-2, 1, 0), 2)):                       # the intensity change: the same two roundings, the fill untouched
        got = R.apply_ref(plain, R.table_of([R.integer_map(roi, offset, flips)], (scale, shift)), roi, fill=-2.5)
        assert torch.equal(A.bits(got), A.bits(A.apply_ref(plain, R.augment_rows([(offset, flips)], (scale, shift)), roi, fill=-2.5)))


def test_quarter_turns_are_rot90():
    x = special_volume((1, 7, 7, 7), 9)
    roi = (7, 7, 7)
    c = 3.0
    for (a, b), sign in itertools.product(((1, 2), (0, 2), (0, 1)), (1.0, -1.0)):
        rot = [[1.0 if r == q else 0.0 for q in range(3)] for r in range(3)]
        rot[a][a], rot[b][b], rot[a][b], rot[b][a] = 0.0, 0.0, -sign, sign
        m = []
        for r in range(3):
            m += rot[r] + [c - sum(rot[r][q] * c for q in range(3))]
        got = R.apply_ref(x, R.table_of([m]), roi)
        # s_a = c - sign (i_b - c), s_b = c + sign (i_a - c): out[.., i_a, .., i_b, ..] = x[.., c - sign (i_b - c), .., c + sign (i_a - c), ..]
        want = torch.rot90(x, -1 if sign > 0 else 1, (1 + a, 1 + b))
        assert torch.equal(A.bits(got), A.bits(want)), ((a, b), sign)
    # the quarter turns of the GPU gate's tables are integer maps, hence permutations of cells or the fill
    for m in R.hand_tables((16, 16, 16))["quarter turns"]:
        assert all(v == math.floor(v) for v in m)
        got = R.apply_ref(R.volume(1), R.table_of([m]), (16, 16, 16), fill=7.0)
        assert set(A.bits(got).flatten().tolist()) <= set(A.bits(R.volume(1)).flatten().tolist()) | {R.f32_bits(7.0)}


# ------------------------------------------------------------------ (d) teeth
@pytest.mark.parametrize("wrong", [dict(lerp_fused=True), dict(order="xyz"), dict(incremental=True)], ids=["fused lerp", "x-y-z order", "incremental"])
def test_a_wrong_arithmetic_differs_on_the_gpu_gates_inputs(wrong):
    roi = (16, 16, 16)
    x = R.volume()
    table = R.table_of(R.hand_tables(roi)["rotation"])
    right, other = R.apply_ref(x, table, roi, fill=-2.5), R.apply_ref(x, table, roi, fill=-2.5, **wrong)
    differing = (A.bits(right) != A.bits(other)).sum().item()
    print(f"{wrong}: {differing} of {right.numel()} cells differ")
    assert differing >= 1
    assert (right - other).abs().max() < 1e-4                                    # ... by roundings: the wrong form is the same geometry


# ------------------------------------------------------------------ (e) draws
KW = dict(rotate=(10, 5, 20), zoom=(0.9, 1.1), isotropic=False, translate=(4, 0.5, 2), prob=0.5, flip_prob=(0.5, 0.25, 1.0), scale=(0.9, 1.1),
          shift=(-0.25, 0.125))
IN_SIZE, ROI = (90, 91, 109), (80, 80, 80)


def is_integer_row(row):
    return all(v == math.floor(v) for v in row[:12].view(torch.float32).tolist())


def test_draws_are_deterministic_differ_between_ranks_and_ignore_the_batch_size():
    a, _ = R.params_ref(5, 3, IN_SIZE, ROI, seed=7, rank=1, **KW)
    again, _ = R.params_ref(5, 3, IN_SIZE, ROI, seed=7, rank=1, **KW)
    assert torch.equal(a, again)
    other_rank, _ = R.params_ref(5, 3, IN_SIZE, ROI, seed=7, rank=2, **KW)
    other_step, _ = R.params_ref(5, 4, IN_SIZE, ROI, seed=7, rank=1, **KW)
    other_seed, _ = R.params_ref(5, 3, IN_SIZE, ROI, seed=8, rank=1, **KW)
    for other in (other_rank, other_step, other_seed):
        assert all(not torch.equal(a[b], other[b]) for b in range(5))
    assert all(not torch.equal(a[b], a[c]) for b, c in itertools.combinations(range(5), 2))
    longer, _ = R.params_ref(9, 3, IN_SIZE, ROI, seed=7, rank=1, **KW)
    assert torch.equal(longer[:5], a)
    assert (a[:, 15] == 0).all() and ((a[:, 14] & ~15) == 0).all() and ((a[:, 14] & 4) == 4).all()        # flip_prob 1.0 on z
    # the affine domain is not the augmentation's: the crop offsets of the two differ somewhere
    aug = A.params_ref(64, 3, IN_SIZE, ROI, seed=7, rank=1)
    aff, _ = R.params_ref(64, 3, IN_SIZE, ROI, seed=7, rank=1, prob=0.0)
    assert not torch.equal(aug[:, :3], aff[:, [3, 7, 11]].view(torch.float32).to(torch.int32))


def test_prob_never_and_always_applies_and_unapplied_rows_are_integer_maps():
    never, _ = R.params_ref(64, 0, IN_SIZE, ROI, seed=3, **dict(KW, prob=0.0))
    always, _ = R.params_ref(64, 0, IN_SIZE, ROI, seed=3, **dict(KW, prob=1.0))
    half, _ = R.params_ref(64, 0, IN_SIZE, ROI, seed=3, **KW)
    assert ((never[:, 14] & 8) == 0).all() and ((always[:, 14] & 8) == 8).all()
    applied = (half[:, 14] & 8) == 8
    assert 12 <= applied.sum() <= 52                                             # 32 +- 5 sigma (sigma 4)
    for b in range(64):
        assert is_integer_row(never[b]) and not is_integer_row(always[b])
        assert is_integer_row(half[b]) == (not applied[b])
        assert torch.equal(half[b] if applied[b] else never[b], (always if applied[b] else half)[b])        # the same draws either way
        # an unapplied row IS the augmentation row of its crop and flips
        flips = int(never[b, 14]) & 7
        m = never[b, :12].view(torch.float32).tolist()
        offset = [int(m[4 * a + 3]) - (ROI[a] - 1 if (flips >> a) & 1 else 0) for a in range(3)]
        assert all(0 <= o <= n - s for o, n, s in zip(offset, IN_SIZE, ROI))
        assert torch.equal(never[b, :12], R.table_of([R.integer_map(ROI, offset, flips)])[0, :12])


def test_drawn_maps_stay_in_their_ranges():
    kw = dict(KW, prob=1.0, flip_prob=(0, 0, 0))
    _, exact = R.params_ref(256, 1, IN_SIZE, ROI, seed=5, **kw)
    M = exact.view(256, 3, 4)[:, :, :3]
    zoom = M.norm(dim=1)                                                         # the columns of R diag(1 / z) have length 1 / z_b
    assert (zoom >= 1 / 1.1 - 1e-12).all() and (zoom <= 1 / 0.9 + 1e-12).all()
    assert ((M / zoom[:, None, :]) @ (M / zoom[:, None, :]).transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-12      # a rotation
    iso, _ = R.params_ref(64, 1, IN_SIZE, ROI, seed=5, **dict(kw, isotropic=True))
    zi = iso[:, :12].view(torch.float32).view(64, 3, 4)[:, :, :3].double().norm(dim=1)
    assert (zi.max(dim=1).values - zi.min(dim=1).values).max() < 1e-6            # one zoom for the three axes
    # the centre of the window lands at crop offset + translation + (S - 1) / 2
    c = torch.tensor([(s - 1) / 2.0 for s in ROI], dtype=torch.float64)
    centre = (exact.view(256, 3, 4)[:, :, :3] @ c) + exact.view(256, 3, 4)[:, :, 3]
    lo = c - torch.tensor(KW["translate"], dtype=torch.float64)
    hi = c + torch.tensor([n - s for n, s in zip(IN_SIZE, ROI)], dtype=torch.float64) + torch.tensor(KW["translate"], dtype=torch.float64)
    assert (centre >= lo - 1e-9).all() and (centre <= hi + 1e-9).all()


# ------------------------------------------------------------------ (f) refusals
def make_config(**kw):
    from neurovit_amd.augment import AffineConfig
    d3 = lambda *v: (ctypes.c_double * 3)(*v)
    cfg = AffineConfig(ctypes.sizeof(AffineConfig), (ctypes.c_int * 3)(90, 90, 90), (ctypes.c_int * 3)(80, 80, 80), d3(10, 10, 10), 0.9, 1.1, 1,
                       d3(4, 4, 4), 1.0, d3(0, 0, 0), 1.0, 1.0, 0.0, 0.0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib
    from neurovit_amd.augment import AffineConfig
    assert ctypes.sizeof(AffineConfig) == 152
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    i3, d3 = lambda *v: (ctypes.c_int * 3)(*v), lambda *v: (ctypes.c_double * 3)(*v)
    params = lambda cfg, B=2, rank=0, out=fake: lib.nv_affine_params(ctypes.byref(cfg) if cfg is not None else None, 1, 0, rank, B, out, None)
    nan, inf = float("nan"), float("inf")
    assert params(None) == -1
    assert params(make_config(), out=None) == -1
    assert params(make_config(), B=0) == -1
    assert params(make_config(), rank=-1) == -1
    assert params(make_config(struct_size=148)) == -1 and "struct_size" in _cabi.last_error()
    assert params(make_config(roi=i3(80, 91, 80))) == -1 and "larger" in _cabi.last_error()
    assert params(make_config(roi=i3(80, -1, 80))) == -1 and "positive" in _cabi.last_error()
    assert params(make_config(in_size=i3(-90, 90, 90))) == -1
    for bad in (d3(0, 180.5, 0), d3(-181, 0, 0), d3(0, 0, nan), d3(inf, 0, 0)):
        assert params(make_config(rotate_deg=bad)) == -1 and "rotate_deg" in _cabi.last_error()
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (1.2, 1.1), (1.0, 16.5), (nan, 1.0), (1.0, nan)):
        assert params(make_config(zoom_lo=lo, zoom_hi=hi)) == -1 and "zoom" in _cabi.last_error(), (lo, hi)
    for bad in (d3(-0.5, 0, 0), d3(0, inf, 0), d3(0, 0, nan)):
        assert params(make_config(translate=bad)) == -1 and "translate" in _cabi.last_error()
    for bad in (-0.1, 1.5, nan):
        assert params(make_config(prob=bad)) == -1 and "prob" in _cabi.last_error()
        assert params(make_config(flip_prob=d3(0, bad, 0))) == -1 and "probability" in _cabi.last_error()
    assert params(make_config(scale_lo=1.5, scale_hi=0.5)) == -1 and "lo <= hi" in _cabi.last_error()
    assert params(make_config(shift_lo=0.5, shift_hi=-0.5)) == -1
    assert params(make_config(shift_hi=inf)) == -1

    strides = (ctypes.c_long * 5)(729000, 8100, 90, 1, 1)
    sp = ctypes.cast(strides, ctypes.c_void_p)
    p3 = lambda *v: ctypes.cast(i3(*v), ctypes.c_void_p)
    far = 1 << 40

    def apply(src=fake, st=sp, B=2, in3=(90, 90, 90), T=1, tab=fake, roi3=(80, 80, 80), out=far):
        return lib.nv_affine_apply(src, st, B, p3(*in3), T, tab, p3(*roi3), 0.0, out, None)
    for kw in (dict(src=None), dict(st=None), dict(tab=None), dict(out=None), dict(B=0), dict(B=-3), dict(T=0)):
        assert apply(**kw) == -1, kw
    assert apply(roi3=(80, 80, 91)) == -1 and "larger" in _cabi.last_error()
    assert apply(roi3=(0, 80, 80)) == -1 and "positive" in _cabi.last_error()
    assert apply(in3=(90, -90, 90)) == -1 and "positive" in _cabi.last_error()
    assert apply(out=far + 4) == -1 and "16-byte" in _cabi.last_error()
    assert apply(in3=(9000, 9000, 9000), roi3=(80, 8000, 8000), T=64) == -1 and "beyond one launch" in _cabi.last_error()
    # an out inside, at the start of, at the last element of or around the memory src reaches is refused; one that ends where src begins is not the issue here
    reach = 4 * (729000 + 89 * 8100 + 89 * 90 + 89)          # byte offset of the last element of src
    for out in (fake, fake + 4096, fake + reach - reach % 16, fake - 16):
        assert apply(out=out) == -1 and "aliases" in _cabi.last_error(), out


def test_volume_affine_refuses_bad_configurations():
    from neurovit_amd.augment import VolumeAffine
    nan, inf = float("nan"), float("inf")
    for kw in (dict(roi=0), dict(roi=(8, -1, 8)), dict(roi=(8, 8)), dict(rotate=181), dict(rotate=(0, -180.5, 0)), dict(rotate=nan), dict(rotate=(1, 2)),
               dict(zoom=(0, 1)), dict(zoom=(1.2, 1.1)), dict(zoom=(1, 17)), dict(zoom=(nan, 1)), dict(translate=-1), dict(translate=(0, inf, 0)),
               dict(translate=nan), dict(prob=1.5), dict(prob=-0.1), dict(prob=nan), dict(flip_prob=(0, 2, 0)), dict(scale=(1.5, 0.5)), dict(shift=(0, inf)),
               dict(seed=-1), dict(seed=2 ** 64), dict(rank=-1), dict(rank=2 ** 31)):
        with pytest.raises(ValueError):
            VolumeAffine(**{"roi": 8, **kw})
    for kw in (dict(roi=8.0), dict(rotate=("1", "2", "3")), dict(rotate=(1, "2", 3)), dict(rotate=True), dict(zoom=1.1), dict(zoom=("a", 1)),
               dict(zoom=(True, 1)), dict(zoom=(1, 1, 1)), dict(isotropic=1), dict(isotropic=None), dict(translate=(1, "2", 3)), dict(prob="1"), dict(prob=True),
               dict(flip_prob=("a", 0, 0)), dict(scale=1.0), dict(seed=1.0), dict(seed=True), dict(rank="0")):
        with pytest.raises(TypeError):
            VolumeAffine(**{"roi": 8, **kw})
    full = VolumeAffine((8, 9, 10), rotate=10, zoom=(0.9, 1.1), isotropic=False, translate=(4, 0, 0.5), prob=0.5, flip_prob=(0.5, 0, 0), scale=(0.9, 1.1),
                        shift=(-0.1, 0.1), fill=-1, seed=3, rank=2)
    assert full.roi == (8, 9, 10) and full.rotate == (10.0, 10.0, 10.0) and full.zoom == (0.9, 1.1) and full.translate == (4.0, 0.0, 0.5)
    assert full.isotropic is False and full.prob == 0.5 and full.fill == -1.0 and (full.seed, full.rank, full.step, full.last_params) == (3, 2, 0, None)


def test_volume_affine_names_itself_in_the_refusals_it_shares():
    """the checks VolumeAffine shares with VolumeAugment (a triple, a range, the step) report under the class the caller used"""
    from neurovit_amd.augment import VolumeAffine
    for refused in (lambda: VolumeAffine(8, rotate=(1, 2)), lambda: VolumeAffine(8, scale=(2, 1)), lambda: VolumeAffine(8).params(2, -1)):
        with pytest.raises((TypeError, ValueError)) as err:
            refused()
        assert "VolumeAffine" in str(err.value) and "VolumeAugment" not in str(err.value)


def test_the_windowed_transforms_share_one_base():
    from neurovit_amd import augment
    base = augment.VolumeAugment.__mro__[1]
    assert base is not object and base is augment.VolumeAffine.__mro__[1]
    for cls in (augment.VolumeAugment, augment.VolumeAffine):
        assert isinstance(cls(8), base)
        assert not {"__call__", "apply", "is_identity", "_check_input"} & set(vars(cls)), cls.__name__
        assert all(callable(getattr(cls, name)) for name in ("__call__", "apply", "is_identity", "_check_input", "params", "_transforms_off"))


def test_volume_affine_refuses_bad_inputs_before_any_device_work():
    from neurovit_amd.augment import VolumeAffine, VolumeAugment, VolumeMix
    aff = VolumeAffine(8, rotate=10)
    x = torch.randn(2, 9, 9, 9)
    table = torch.zeros(2, 16, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aff(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aff.apply(x, table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aff.params(2, 0, device="cpu")
    with pytest.raises(ValueError, match="requires grad"):
        aff(x.clone().requires_grad_())
    with pytest.raises(TypeError, match="dtype"):
        aff(x.double())
    with pytest.raises(TypeError, match="tensor"):
        aff([1, 2])
    with pytest.raises(ValueError, match="larger than the input"):
        aff(torch.randn(2, 9, 7, 9))
    with pytest.raises(ValueError, match="expected"):
        aff(torch.randn(9, 9, 9))
    with pytest.raises(ValueError, match="larger than the input"):
        aff.params(2, 0, in_size=(9, 7, 9))
    with pytest.raises(ValueError, match="B must be"):
        aff.params(0, 0)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="step"):
            aff.params(2, bad)
    with pytest.raises(TypeError, match="step"):
        aff.params(2, 1.0)
    # what the identity is: no transform on (or a probability of zero) and a window as large as the input
    assert VolumeAffine(9, rotate=10, prob=0.0).is_identity(x)
    assert VolumeAffine(9).is_identity(x) and not VolumeAffine(9, rotate=1).is_identity(x) and not VolumeAffine(8).is_identity(x)
    assert not VolumeAffine(9, prob=0.0, flip_prob=(0, 0, 0.5)).is_identity(x)
    # VolumeMix takes both kinds, and keeps its words for anything else
    mix = VolumeMix(mixup_alpha=0.5)
    for bad in (object(), "augment", VolumeAffine):
        with pytest.raises(TypeError, match="augment must be a VolumeAugment"):
            mix(x, augment=bad)
        with pytest.raises(TypeError, match="augment must be a VolumeAugment"):
            mix.apply(x, torch.zeros(2, 12, dtype=torch.int32), augment=bad, augment_params=table)
    for good in (aff, VolumeAugment(8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mix(x, augment=good)
    with pytest.raises(ValueError, match="come together"):
        mix.apply(x, torch.zeros(2, 12, dtype=torch.int32), augment=aff)


def test_trainer_reads_the_affine_keys():
    from neurovit_amd.augment import VolumeAffine, VolumeAugment
    from neurovit_amd.trainer import Trainer
    base = dict(TRAINING_VIT_INPUT_SIZE=32)
    on = dict(base, DATASET_TRANSFORMS=True)
    assert Trainer.augment_from_config(dict(base, AUGMENT_ROTATE_DEG=10)) is None                  # the switch is DATASET_TRANSFORMS
    assert type(Trainer.augment_from_config(on)) is VolumeAugment                                   # none of the keys: nothing changes
    assert type(Trainer.augment_from_config(dict(on, AUGMENT_MAX_SHIFT=2, AUGMENT_ROTATE_DEG=None))) is VolumeAugment
    for key, value in (("AUGMENT_ROTATE_DEG", 10), ("AUGMENT_ZOOM", (0.9, 1.1)), ("AUGMENT_ZOOM_ISOTROPIC", False), ("AUGMENT_TRANSLATE", (4, 4, 0)),
                       ("AUGMENT_AFFINE_PROB", 0.5)):
        one = Trainer.augment_from_config(dict(on, **{key: value}))
        assert type(one) is VolumeAffine and one.roi == (32, 32, 32), key
        with pytest.raises(ValueError, match="AUGMENT_TRANSLATE"):
            Trainer.augment_from_config(dict(on, AUGMENT_MAX_SHIFT=2, **{key: value}))
    full = Trainer.augment_from_config(dict(on, AUGMENT_ROTATE_DEG=(10, 5, 0), AUGMENT_ZOOM=[0.9, 1.1], AUGMENT_ZOOM_ISOTROPIC=False, AUGMENT_TRANSLATE=4,
                                            AUGMENT_AFFINE_PROB=0.75, AUGMENT_FLIP_PROB=(0.5, 0, 0), AUGMENT_INTENSITY_SCALE=(0.9, 1.1),
                                            AUGMENT_INTENSITY_SHIFT=(-0.5, 0.5), AUGMENT_FILL=-1.0, AUGMENT_SEED=9))
    assert full.rotate == (10.0, 5.0, 0.0) and full.zoom == (0.9, 1.1) and full.isotropic is False and full.translate == (4.0, 4.0, 4.0) and full.prob == 0.75
    assert full.flip_prob == (0.5, 0.0, 0.0) and full.shift == (-0.5, 0.5) and full.fill == -1.0 and (full.seed, full.rank) == (9, 0)
    assert abs(full.scale[0] - 0.9) < 1e-7
    with pytest.raises(ValueError):
        Trainer.augment_from_config(dict(on, AUGMENT_ROTATE_DEG=200))
    with pytest.raises(TypeError):
        Trainer.augment_from_config(dict(on, AUGMENT_ZOOM_ISOTROPIC="yes"))
    with pytest.raises(TypeError):
        Trainer.augment_from_config(dict(on, AUGMENT_ZOOM=1.1))
