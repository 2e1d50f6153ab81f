"""CPU restatement of the weight average (neurovit_amd.ModelEma, csrc/ema.hip), shared by tests/test_ema_cpu.py and tests/test_ema_gpu.py:

  * the decay rule in Python floats (double): d_t = min(decay, (1 + t) / (10 + t)) with warmup (timm), d_t ** update_every on the calls that
    average, and the fp32 weight float32(1 - d) the kernel gets;
  * the update e + (p - e) * w in fp32, every operation rounded on its own - as a torch expression and per operation in numpy.float32;
  * the recurrence over a list of parameter snapshots, one per update call.
"""
import numpy as np
import torch


def decay_at(t, decay, warmup=True, update_every=1):
    """decay of the averaging on update call t >= 1 (double)"""
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return d ** update_every


def weight32(d):
    """numpy.float32(1 - d): the subtraction in double, one rounding"""
    return np.float32(1.0 - d)


def update(e, p, w):
    """the torch expression on fp32 CPU tensors; w: a float32 value (numpy.float32 or the Python float of one)"""
    assert e.dtype == torch.float32 and p.dtype == torch.float32 and not e.is_cuda and not p.is_cuda
    return e + (p - e) * float(w)


def update_np(e, p, w):
    """the same, one numpy.float32 operation at a time"""
    e, p, w = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(w)
    with np.errstate(all="ignore"):
        diff = (p - e).astype(np.float32)
        prod = (diff * w).astype(np.float32)
        return (e + prod).astype(np.float32)


def two_product(e, p, d):
    """the form the kernel does NOT use: float32(d) * e + float32(1 - d) * p, the two factors rounded independently"""
    return e * float(np.float32(d)) + p * float(np.float32(1.0 - d))


def replay(start, snapshots, decay, warmup=True, update_every=1, first_call=1):
    """The average after update calls first_call, first_call + 1, ... that saw the parameter arenas `snapshots` (CPU fp32), from
    `start`: -> (average, number of the last call)."""
    e, t = start.clone(), first_call - 1
    for p in snapshots:
        t += 1
        if t % update_every == 0:
            e = update(e, p, weight32(decay_at(t, decay, warmup, update_every)))
    return e, t


def same_bits(a, b):
    """fp32 tensors equal bit for bit, except that a NaN matches any NaN (the sign and payload of a generated NaN are the processor's)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb]))
