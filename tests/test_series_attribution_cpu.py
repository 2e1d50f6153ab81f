"""CPU checks of the 4D model's series attribution (no GPU): the C-ABI pieces csrc/series_attr.hip adds within revision 8
(nv_gradcam_reduce_grouped, nv_series_map_to_volumes, nv_series_leave_one_out, nv_temporal_grad_x_input and the two workspace queries),
and the CPU restatements of tests/series_attribution_ref.py that the GPU tests (tests/test_series_attribution_gpu.py) measure against:

  scope VOLUME   the series restatement equals tests/test_attribution_volume_cpu.py's `restate` applied to each (b, t), bit for bit;
  scope SERIES   it equals `restate`'s normalisation and cut applied to the flattened [B, T N] map, and its cut on T N cells equals
                 torch.quantile(interpolation='linear') in double;
  temporal       the leave-one-out table and grad x input, run through oracle.ref_cpu.temporal_head, equal plain torch autograd / a
                 per-timepoint loop on that composition;
  precondition   every volume of every module case of the GPU file has a raw Grad-CAM range well above the 1e-8 of the normalisation
                 (oracle composition, fp32), and the ranges of a sample's timepoints differ.
"""
import ctypes

import pytest
import torch

import series_attribution_ref as R
import weights as W
from oracle import ref_cpu
from test_attribution_volume_cpu import minmax_reciprocal, quantile_cut, relu_maps, restate

KEEPS = (5, 20, 37.5, 100)
SHAPES = [(1, (4, 4, 4), (32,) * 3), (3, (2, 2, 2), (16,) * 3), (5, (4, 6, 5), (20, 36, 45)), (8, (16, 16, 16), (32,) * 3)]


def i3(*v):
    arr = (ctypes.c_int * 3)(*v)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    names = ("nv_gradcam_reduce_grouped", "nv_series_map_to_volumes", "nv_series_leave_one_out", "nv_temporal_grad_x_input",
             "nv_gradcam_grouped_workspace_bytes", "nv_series_map_to_volumes_workspace_bytes")
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in names:
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    # new symbols only: the revision stays; the grouped reduction takes the existing argument list plus `group`
    assert _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8
    args = list(_cabi.lib.protos["nv_gradcam_reduce"][1])
    assert _cabi.lib.protos["nv_gradcam_reduce_grouped"][1] == args[:5] + [ctypes.c_int] + args[5:]
    assert _cabi.lib.protos["nv_series_map_to_volumes"][1][7] is ctypes.c_double
    header = open(_cabi.HEADER).read()
    for constant in ("NV_SERIES_SCOPE_SERIES 0", "NV_SERIES_SCOPE_VOLUME 1", "NV_SERIES_LAYOUT_SERIES 0", "NV_SERIES_LAYOUT_FRAMES 1"):
        assert "#define " + constant in header
    from neurovit_amd import ops
    assert ops.SERIES_SCOPES == {"series": 0, "volume": 1} and ops.SERIES_LAYOUTS == {"series": 0, "frames": 1}


def test_argument_checks_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib
    fake, big = 4096, 1 << 30                              # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    SERIES, VOLUME, FRAMES = 0, 1, 1
    _g, g4 = i3(4, 4, 4)
    _s, s32 = i3(32, 32, 32)
    _h, g16 = i3(16, 16, 16)

    def series(maps=fake, B=1, T=3, grid=g4, size=s32, scope=SERIES, keep=5.0, layout=SERIES, out=fake, ws=fake, nbytes=big):
        return lib.nv_series_map_to_volumes(maps, B, T, grid, size, 1, scope, keep, layout, out, ws, nbytes, None)
    assert lib.nv_series_map_to_volumes_workspace_bytes(2, 3, g4, SERIES) == (2 * 2 * 3 * 64 + 2) * 4
    assert lib.nv_series_map_to_volumes_workspace_bytes(2, 3, g4, VOLUME) == (2 * 2 * 3 * 64 + 6) * 4
    assert lib.nv_series_map_to_volumes_workspace_bytes(2, 0, g4, SERIES) < 0 and lib.nv_series_map_to_volumes_workspace_bytes(2, 65, g4, SERIES) < 0
    assert series(T=0) == -1 and "timepoints" in _cabi.last_error()
    assert series(T=65) == -1 and "timepoints" in _cabi.last_error()
    assert series(T=65, scope=VOLUME) == -1
    # T N = 32769 = 9 x 11 x 331 cells, one beyond the limit: 9 timepoints of a 1 x 11 x 331 grid (3641 <= 4096 cells per volume); 8 x 16^3 is the limit
    _e, g3641 = i3(1, 11, 331)
    assert series(T=9, grid=g3641) == -1 and "scope VOLUME" in _cabi.last_error() and "32769" in _cabi.last_error() and "32768" in _cabi.last_error()
    assert series(T=9, grid=g3641, scope=VOLUME, layout=FRAMES, nbytes=8) == -1 and "workspace" in _cabi.last_error()     # the limit is scope SERIES's
    assert series(T=9, grid=g16) == -1 and "scope VOLUME" in _cabi.last_error()
    _o, odd = i3(1, 1, 32769)
    assert series(T=1, grid=odd) == -1                     # one volume of 32769 cells: beyond the per-volume limit already
    assert series(T=8, grid=g16, nbytes=8) == -1 and "workspace" in _cabi.last_error()          # at the limit: passes on to the next check
    assert series(T=9, grid=g16, scope=VOLUME, layout=FRAMES, nbytes=8) == -1 and "workspace" in _cabi.last_error()
    assert series(maps=None) == -1 and series(out=None) == -1 and series(ws=None) == -1 and series(grid=None) == -1 and series(size=None) == -1
    assert series(out=fake + 4) == -1 and "aligned" in _cabi.last_error()
    assert series(ws=fake + 8) == -1 and "aligned" in _cabi.last_error()
    assert series(keep=101.0) == -1 and "keep_percent" in _cabi.last_error()
    assert series(scope=2) == -1 and series(layout=2) == -1 and series(B=0) == -1
    assert series(nbytes=8) == -1 and "workspace" in _cabi.last_error()
    _b, s4k = i3(32, 12000, 12000)                         # tables of the y and z taps beyond one workgroup's LDS
    assert series(size=s4k) == -1 and "tables" in _cabi.last_error()

    def grouped(act=fake, grad=fake, V=6, n=65, d=128, group=3, cam=fake, ws=fake, nbytes=big):
        return lib.nv_gradcam_reduce_grouped(act, grad, V, n, d, group, cam, None, ws, nbytes, None)
    assert lib.nv_gradcam_grouped_workspace_bytes(6, 65, 4) < 0 and lib.nv_gradcam_grouped_workspace_bytes(6, 65, 0) < 0
    assert lib.nv_gradcam_grouped_workspace_bytes(6, 65, 1) == lib.nv_gradcam_per_volume_workspace_bytes(6, 65)
    assert lib.nv_gradcam_grouped_workspace_bytes(6, 65, 6) == lib.nv_gradcam_workspace_bytes(6, 65)
    assert grouped(group=4) == -1 and "groups of 4" in _cabi.last_error()                     # V % group != 0
    assert grouped(group=0) == -1 and grouped(act=None) == -1 and grouped(grad=None) == -1 and grouped(cam=None) == -1 and grouped(ws=None) == -1
    assert grouped(d=100) == -1 and grouped(nbytes=8) == -1 and grouped(act=fake + 4) == -1

    assert lib.nv_series_leave_one_out(None, fake, 1, 3, fake, None) == -1 and lib.nv_series_leave_one_out(fake, None, 1, 3, fake, None) == -1
    assert lib.nv_series_leave_one_out(fake, fake, 1, 3, None, None) == -1
    assert lib.nv_series_leave_one_out(fake, fake, 1, 0, fake, None) == -1 and lib.nv_series_leave_one_out(fake, fake, 1, 65, fake, None) == -1
    assert lib.nv_series_leave_one_out(fake, fake, 0, 3, fake, None) == -1 and lib.nv_series_leave_one_out(fake, fake, 1, 3, fake + 2, None) == -1
    assert lib.nv_temporal_grad_x_input(None, fake, 1, 3, fake, None) == -1 and lib.nv_temporal_grad_x_input(fake, None, 1, 3, fake, None) == -1
    assert lib.nv_temporal_grad_x_input(fake, fake, 1, 3, None, None) == -1
    assert lib.nv_temporal_grad_x_input(fake, fake, 1, 0, fake, None) == -1 and lib.nv_temporal_grad_x_input(fake, fake, 1, 65, fake, None) == -1
    assert lib.nv_temporal_grad_x_input(fake, fake, 0, 3, fake, None) == -1 and lib.nv_temporal_grad_x_input(fake, fake, 1, 3, fake + 1, None) == -1


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("T,grid,size", SHAPES, ids=[f"T{s[0]}-{s[1][0]}x{s[1][1]}x{s[1][2]}" for s in SHAPES])
def test_series_restatement_against_the_volume_restatement(T, grid, size, keep):
    N = grid[0] * grid[1] * grid[2]
    B = 2
    raw = (relu_maps(B * T, N, 13 * N + T) * torch.linspace(0.05, 9.0, B * T)[:, None]).reshape(B, T, N)      # the timepoints' ranges differ
    assert float((raw == 0).float().mean()) > 0.3
    # scope VOLUME: `restate` on each (b, t), bit for bit
    norm, cuts, sparse, vols = R.restate_series(raw, grid, size, keep, "volume")
    for b in range(B):
        for t in range(T):
            one = minmax_reciprocal(raw[b, t][None])
            c, sp, v = restate(one, grid, size, keep)
            assert torch.equal(norm[b, t], one[0]) and torch.equal(cuts[b, t], c[0]) and torch.equal(sparse[b, t], sp[0]) and torch.equal(vols[b, t], v[0])
    # scope SERIES: `restate`'s normalisation and cut on the flattened [B, T N] map
    norm, cuts, sparse, vols = R.restate_series(raw, grid, size, keep, "series")
    flat = minmax_reciprocal(raw.reshape(B, T * N))
    assert torch.equal(norm.reshape(B, T * N), flat)
    assert (norm.reshape(B, -1).amin(1) == 0).all() and (norm.reshape(B, -1).amax(1) > 0.999).all()
    for b in range(B):
        want = torch.quantile(flat[b].double(), 1.0 - keep / 100.0, interpolation='linear').to(torch.float32)
        assert torch.equal(quantile_cut(flat[b], keep), want) and torch.equal(cuts[b], want), (T, grid, keep)
        kept = flat[b] >= want
        assert torch.equal(sparse[b].reshape(-1), torch.where(kept, flat[b], torch.zeros(())))
        for t in range(T):                                  # the upsampling is the volume restatement's, on the jointly thresholded grid
            _, _, v = restate(sparse[b, t][None], grid, size, 100)
            assert torch.equal(vols[b, t], v[0])
    if T > 1:                                               # why the scope exists: per volume every timepoint reaches 1, jointly only the strongest
        per_volume = R.restate_series(raw, grid, size, keep, "volume")[0]
        assert (per_volume.amax(2) > 0.999).all() and int((norm.amax(2) > 0.999).sum()) == B


def small_head(seed, ff=16):
    """a state_dict of the temporal head with the reference's keys (feed-forward width ff) and a z [B, T, 2] to run it on"""
    g = torch.Generator().manual_seed(seed)
    pre = "temporal_transformer.transformer.layers.0."
    shapes = {pre + "self_attn.in_proj_weight": (6, 2), pre + "self_attn.in_proj_bias": (6,), pre + "self_attn.out_proj.weight": (2, 2),
              pre + "self_attn.out_proj.bias": (2,), pre + "linear1.weight": (ff, 2), pre + "linear1.bias": (ff,), pre + "linear2.weight": (2, ff),
              pre + "linear2.bias": (2,), pre + "norm1.weight": (2,), pre + "norm1.bias": (2,), pre + "norm2.weight": (2,), pre + "norm2.bias": (2,),
              "projection_head.projection_head.weight": (2, 2), "projection_head.projection_head.bias": (2,)}
    return {k: (1.0 + 0.1 * torch.randn(s, generator=g) if k.endswith(("norm1.weight", "norm2.weight")) else 0.7 * torch.randn(s, generator=g))
            for k, s in shapes.items()}


@pytest.mark.parametrize("B,T", [(1, 3), (2, 4), (3, 7)])
@pytest.mark.parametrize("kind", ["prob", "logit"])
def test_temporal_restatements_against_autograd_on_the_oracle_head(B, T, kind):
    sd = small_head(5 + T)
    g = torch.Generator().manual_seed(17 * B + T)
    z, z_base = torch.randn(B, T, 2, generator=g), torch.randn(2, generator=g)
    table = R.leave_one_out_table(z, z_base)
    assert table.shape == (B * (T + 1), T, 2)
    logits, cls, dx = R.head_seed(sd, z)
    assert torch.equal(logits, ref_cpu.temporal_head(sd, z)) and torch.equal(cls, logits.argmax(1))
    occ = R.temporal_occlusion(sd, z, z_base, cls, kind)
    gxi = R.grad_x_input(dx, z)
    for b in range(B):
        assert torch.equal(table[b * (T + 1)], z[b])
        leaf = z[b:b + 1].clone().requires_grad_(True)
        out = ref_cpu.temporal_head(sd, leaf)
        (want_dx,) = torch.autograd.grad(out[0, cls[b]], leaf)                # plain autograd on the composition, sample by sample
        assert torch.allclose(dx[b], want_dx[0], rtol=1e-5, atol=1e-7)
        want = sum(want_dx[0, :, c] * z[b, :, c] for c in range(2))
        assert torch.allclose(gxi[b], want, rtol=1e-5, atol=1e-7)
        base = R.class_score(out.detach(), cls[b:b + 1], kind)[0]
        for t in range(T):
            seq = z[b:b + 1].clone()
            seq[0, t] = z_base
            assert torch.equal(table[b * (T + 1) + 1 + t], seq[0])
            with torch.no_grad():
                s = R.class_score(ref_cpu.temporal_head(sd, seq), cls[b:b + 1], kind)[0]
            assert torch.allclose(occ[b, t], base - s, rtol=1e-5, atol=1e-6)
    # a baseline equal to the timepoint changes nothing: that entry of the occlusion is exactly 0
    same = R.temporal_occlusion(sd, z[:1, :1].repeat(1, T, 1), z[0, 0], cls[:1], kind)
    assert (same == 0).all()


def test_module_cases_have_live_gradcam_maps(tmp_path):
    """precondition of the GPU module tests: the oracle's raw Grad-CAM range of every VOLUME of every case is above GRADCAM_RAW_FLOOR
    (so a normalised map peaks above 0.9 per volume and per sample, and the scopes differ), for every class the tests explain"""
    for T, B, seed, head in R.MODULE_CASES:
        model, cfg4 = R.micro_4d_model(tmp_path, "cpu", head)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        series = W.make_volume((B, R.S, R.S, R.S, T), seed)
        for target in (None, torch.zeros(B, dtype=torch.long), torch.ones(B, dtype=torch.long), torch.arange(B) % 2, 1 - torch.arange(B) % 2):
            o = R.oracle_series(sd, cfg4, series, False, target=target, want=("hook",))
            cam = R.gradcam_raw(o["act"], o["grad"])
            assert (cam.amin(dim=1) == 0).all() and (cam.amax(dim=1) > R.GRADCAM_RAW_FLOOR).all(), (T, B, target, cam.amax(dim=1))
            per_volume = cam.amax(dim=1).reshape(B, T)
            assert (per_volume.amax(1) > 1.2 * per_volume.amin(1)).all()          # the timepoints differ: scope "series" is not scope "volume"
