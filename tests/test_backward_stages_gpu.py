"""The staged, unjoined backward against the one-call backward, bit for bit, at an ODD depth.

The auxiliary (weight-gradient) stream works one layer behind the main stream on buffers that exist twice, one copy for even and one
for odd layers.  A backward run stage by stage with join_aux=False hands every cross-call dependency to the next call: the layer whose
LN1-backward partials still wait for their reduction, and the event behind which the next call may reuse a buffer copy.  At depth 3
an even-layer copy and an odd-layer copy both cross a call boundary (tests/test_dp_gpu.py reaches this code at depth 2 only).  A wrong
copy index, a lost reduction or a lost dependency changes bits of the gradient arena: both routes issue the same kernels on the same
data, so the gate is torch.equal - on the fp32 arena and on the 16-bit mirror the weight-gradient GEMMs write.
"""
import pytest
import torch

import weights as W

pytestmark = pytest.mark.gpu
CFG = dict(W.MICRO, depth=3)        # 32^3 volume, patch 8, dim 128, heads 2, mlp 256
B = 2
DROPOUT = (0.1, 0.1, 1234)
LAST = CFG["depth"] + 1


@pytest.fixture(scope="module")
def setup():
    from neurovit_amd import engine
    from neurovit_amd._cabi import require_gpu
    from oracle import ref_cpu
    require_gpu()
    cfg = engine.make_config(**CFG)
    off, num, total = engine.param_layout(cfg)
    sd = W.make_tensors(W.vit_param_spec(**CFG), 5)
    arena = torch.zeros(total)
    for v, o, n in zip(sd.values(), off, num):
        arena[o:o + n] = v.reshape(-1)
    params = arena.cuda()
    S = CFG["image_size"]
    video = ref_cpu.fmri_to_video(W.make_volume((B, S, S, S), 6).cuda())
    dlogits = torch.tensor([[0.3, -0.3], [-0.2, 0.2]], device="cuda")
    return engine, cfg, params, params.to(torch.bfloat16), video, dlogits


def _backward(setup, rows_form, staged, base=None):
    """(fp32 arena, 16-bit arena) of one backward behind a fresh forward; base = arenas to accumulate on top of"""
    engine, cfg, params, params16, video, dlogits = setup
    rt = engine.VitRuntime(cfg)
    rt.forward(video, params, params16, training=True, dropout=DROPOUT, rows_form=rows_form)
    grads = torch.zeros_like(params) if base is None else base[0].clone()
    grads16 = torch.zeros_like(params16) if base is None else base[1].clone()
    for s in (range(LAST + 1) if staged else [None]):
        rt.backward(dlogits, params, params16, grads, accumulate=base is not None, stages=None if s is None else (s, s),
                    join_aux=(s is None or s == LAST), grads16=grads16)
    torch.cuda.synchronize()         # both streams
    return grads, grads16


@pytest.mark.parametrize("rows_form", [1, 2])
def test_staged_unjoined_backward_equals_one_call_bitwise(setup, rows_form):
    whole = _backward(setup, rows_form, staged=False)
    staged = _backward(setup, rows_form, staged=True)
    assert whole[0].abs().sum().item() > 0 and whole[1].float().abs().sum().item() > 0
    assert torch.equal(staged[0], whole[0]), "fp32 gradient arena"
    assert torch.equal(staged[1], whole[1]), "16-bit gradient arena"
    whole2 = _backward(setup, rows_form, staged=False, base=whole)
    staged2 = _backward(setup, rows_form, staged=True, base=whole)
    assert not torch.equal(whole2[0], whole[0])
    assert torch.equal(staged2[0], whole2[0]), "fp32 gradient arena, accumulate"
    assert torch.equal(staged2[1], whole2[1]), "16-bit gradient arena, accumulate"
