"""Training augmentation on the device: per-sample random crop, integer translation, axis flips and an affine intensity change
(`VolumeAugment`), Mixup / CutMix (`VolumeMix`), and a random rotation, zoom and sub-voxel shift (`VolumeAffine`).

The reference has one augmentation switch: `DATASET_TRANSFORMS` makes `ADNIDataset.__getitem__` apply monai's
`RandSpatialCrop(roi_size=(80, 80, 80), random_center=True, random_size=False)` to the z-scored 90^3 volume on the host
(src/data/DatasetADNI.py:27-31, 216-218).  `VolumeAugment` is that crop - and the flips, shifts and intensity changes usually added to
it - as two HIP launches on the batch that is already on the device (csrc/augment.hip): the parameters are drawn on the device from
(seed, rank, step, sample) by the counter hash of the dropout masks, so nothing is read back and the host draws no random number; the
draw rule is part of the C-ABI (include/neurovit_hip.h) and tests/augment_ref.py restates it bit for bit.

`VolumeAugment` moves whole voxels and is exact.  `VolumeAffine` (csrc/affine.hip) is the one transform that resamples: a streaming
gather with trilinear interpolation under a per-sample 3 x 4 map that is drawn and formed on the device in the same way; its fp32
arithmetic is part of the C-ABI and tests/affine_ref.py restates it bit for bit.  A sample it does not turn, zoom or shift is still the
bit copy VolumeAugment would write.  No noise.  No gradient flows through any of them.
"""
from __future__ import annotations

import ctypes
import math
import struct
from typing import Optional, Sequence, Union

import torch

from ._cabi import MIX_COLS, check, lib


class AugmentConfig(ctypes.Structure):
    """struct nv_augment_config (neurovit_hip.h, added within revision 8)."""
    _fields_ = [("struct_size", ctypes.c_int), ("in_size", ctypes.c_int * 3), ("roi", ctypes.c_int * 3), ("max_shift", ctypes.c_int * 3),
                ("flip_prob", ctypes.c_double * 3), ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float), ("shift_lo", ctypes.c_float),
                ("shift_hi", ctypes.c_float)]


# ---------------------------------------------------------------------- what the three transforms check alike (`who` names the class)
def _check_seed_rank(who, seed, rank):
    for name, value, top in (("seed", seed, 2 ** 64), ("rank", rank, 2 ** 31)):
        if isinstance(value, bool) or not isinstance(value, int):
            raise TypeError(f"{who}: {name} must be an integer, got {value!r}")
        if not (0 <= value < top):
            raise ValueError(f"{who}: {name} {value} outside [0, {top})")


def _check_step(who, step) -> int:
    if isinstance(step, bool) or not isinstance(step, int):
        raise TypeError(f"{who}: step must be an integer, got {step!r}")
    if not (0 <= step < 2 ** 64):
        raise ValueError(f"{who}: step {step} outside [0, 2^64)")
    return step


def _at_step(who, obj, step, body):
    """The running-step protocol of a __call__: body(step index) for obj's own counter, which then advances by one, unless `step` is
    given: then for that index, and the counter stays."""
    own = step is None
    out = body(obj.step if own else _check_step(who, step))
    if own:
        obj.step += 1
    return out


def _check_volume(who, what, x, roi=None):
    """x is a float32 batch [B, X, Y, Z(, T)] on the device that needs no gradient; `what` is the transform, for the message; roi: a
    window that must fit into it"""
    if not torch.is_tensor(x):
        raise TypeError(f"{who}: expected a tensor, got {type(x).__name__}")
    if x.dim() not in (4, 5):
        raise ValueError(f"{who}: expected [B, X, Y, Z] or [B, X, Y, Z, T], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"{who}: dtype {x.dtype} unsupported (float32)")
    if x.requires_grad:
        raise ValueError(f"{who}: the input requires grad - no gradient flows through the {what} (detach it)")
    if any(n == 0 for n in x.shape):
        raise ValueError(f"{who}: empty input {tuple(x.shape)}")
    if roi is not None and any(s > n for s, n in zip(roi, x.shape[1:4])):
        raise ValueError(f"{who}: roi {roi} is larger than the input {tuple(x.shape[1:4])}")
    if not x.is_cuda:
        raise RuntimeError(f"neurovit_amd.augment.{who}: input must live on the MI355X (cuda) device - there is no CPU fallback")


def _draw_target(who, B, device) -> torch.device:
    """the batch size and the device of a parameter draw"""
    if isinstance(B, bool) or not isinstance(B, int) or B <= 0:
        raise ValueError(f"{who}.params: B must be a positive integer, got {B!r}")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"neurovit_amd.augment.{who}: parameters are drawn on the MI355X (cuda) device - there is no CPU fallback")
    return device


def _check_rows(who, name, rows, B, cols, device) -> torch.Tensor:
    """a parameter table: int32 [B, cols] on x's device"""
    if not (torch.is_tensor(rows) and rows.dtype == torch.int32 and tuple(rows.shape) == (B, cols) and rows.device == device):
        raise ValueError(f"{who}.apply: {name} must be int32 [{B}, {cols}] on {device}")
    return rows.contiguous()


def _run_pass(who, x, roi, fill, out, entry, *tables):
    """The streaming pass `entry` (nv_augment_apply, nv_augment_mix or nv_affine_apply) over x [B, X, Y, Z(, T)] into the dense
    [B, *roi(, T)] batch, under its checked tables in the order of its signature (None: a table the entry point lets be missing)."""
    four_d = x.dim() == 5
    v = x if four_d else x.unsqueeze(-1)
    B, X, Y, Z, T = v.shape
    shape = (B, *roi, T) if four_d else (B, *roi)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == shape and out.device == x.device
              and out.is_contiguous() and out.data_ptr() % 16 == 0):
        raise ValueError(f"{who}.apply: out must be a dense, 16-byte aligned float32 {shape} on {x.device}")
    strides = (ctypes.c_long * 5)(*v.stride())
    in3, roi3 = (ctypes.c_int * 3)(X, Y, Z), (ctypes.c_int * 3)(*roi)
    src = (v.data_ptr(), ctypes.cast(strides, ctypes.c_void_p), B, ctypes.cast(in3, ctypes.c_void_p), T)
    rows = (None if t is None else t.data_ptr() for t in tables)
    with torch.cuda.device(x.device):
        check(getattr(lib, entry)(*src, *rows, ctypes.cast(roi3, ctypes.c_void_p), fill, out.data_ptr(), torch.cuda.current_stream().cuda_stream), entry)
    return out


def _triple(who, value, name, kind):
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        value = (value,) * 3
    try:
        value = tuple(value)
    except TypeError:
        raise TypeError(f"{who}: {name} must be a number or three numbers, got {value!r}") from None
    if len(value) != 3:
        raise ValueError(f"{who}: {name} must have three entries (x, y, z), got {value!r}")
    if kind is int:
        if any(isinstance(v, bool) or not isinstance(v, int) for v in value):
            raise TypeError(f"{who}: {name} must hold integers, got {value!r}")
        return value
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in value):
        raise TypeError(f"{who}: {name} must hold numbers, got {value!r}")
    return tuple(float(v) for v in value)


def _range(who, value, name):
    try:
        lo, hi = (float(v) for v in value)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: {name} must be a pair (lo, hi) of numbers, got {value!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{who}: {name} must be finite, got {value!r}")
    if lo > hi:
        raise ValueError(f"{who}: {name} has lo > hi: {value!r}")
    as_f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]      # what the kernel sees
    return as_f32(lo), as_f32(hi)


class _WindowTransform:
    """What VolumeAugment and VolumeAffine share: a window `roi` cut from the volume per sample, flips, an intensity change, and the two
    launches - `params` draws a table of `_cols` int32 columns per sample (entry point `_draw`), `apply` is one streaming pass under
    such a table (entry point `_pass`; `_rows` is its name in the messages).  A subclass checks its own options between `_set_window`
    and `_set_shared`, says in `_transforms_off` whether all of them are off, and builds its ctypes config in `_config`."""
    _cols = _rows = _draw = _pass = None

    @property
    def _who(self) -> str:
        return type(self).__name__

    def _set_window(self, roi):
        self.roi = _triple(self._who, roi, "roi", int)
        if any(s <= 0 for s in self.roi):
            raise ValueError(f"{self._who}: roi must be positive, got {self.roi}")

    def _set_flips(self, flip_prob):
        self.flip_prob = _triple(self._who, flip_prob, "flip_prob", float)
        if any(not (0.0 <= p <= 1.0) for p in self.flip_prob):
            raise ValueError(f"{self._who}: flip probabilities must lie in [0, 1], got {self.flip_prob}")

    def _set_shared(self, scale, shift, fill, seed, rank):
        self.scale = _range(self._who, scale, "scale")
        self.shift = _range(self._who, shift, "shift")
        self.fill = float(fill)
        _check_seed_rank(self._who, seed, rank)
        self.seed, self.rank = seed, rank
        self.step = 0                      # the step index the next __call__ without `step=` draws for
        self.last_params: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ checks
    def _shared_off(self) -> bool:
        return all(p == 0.0 for p in self.flip_prob) and self.scale == (1.0, 1.0) and self.shift == (0.0, 0.0)

    def _check_input(self, x: torch.Tensor):
        _check_volume(self._who, "augmentation", x, self.roi)

    def is_identity(self, x: torch.Tensor) -> bool:
        """No transform is on and the roi is the input's spatial size: __call__ returns x itself."""
        return self._transforms_off() and tuple(x.shape[1:4]) == self.roi

    # ------------------------------------------------------------------ the two launches
    def params(self, B: int, step: int, in_size: Optional[Sequence[int]] = None, device=None) -> torch.Tensor:
        """The table for step `step`, int32 [B, 8] (VolumeAugment) or [B, 16] (VolumeAffine) on the device; the class says what a row
        holds.  in_size: (X, Y, Z) of the volumes the window is cut from (default: the roi itself - no room to crop)."""
        step = _check_step(self._who, step)
        in_size = self.roi if in_size is None else _triple(self._who, in_size, "in_size", int)
        if any(s > n for s, n in zip(self.roi, in_size)):
            raise ValueError(f"{self._who}: roi {self.roi} is larger than the input {tuple(in_size)}")
        device = _draw_target(self._who, B, device)
        out = torch.empty((B, self._cols), dtype=torch.int32, device=device)
        cfg = self._config(in_size)
        with torch.cuda.device(device):
            check(getattr(lib, self._draw)(ctypes.byref(cfg), self.seed, step, self.rank, B, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  self._draw)
        return out

    def apply(self, x: torch.Tensor, params: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B, X, Y, Z] or [B, X, Y, Z, T] float32 on the device, dense or a strided view; params: the int32 table (as `params` returns
        it, or written by hand: rows may hold anything).  Returns the dense [B, Sx, Sy, Sz(, T)] batch; a caller-supplied `out` of that
        shape is dense and, for the gather pass of a VolumeAffine, must not overlap x."""
        self._check_input(x)
        params = _check_rows(self._who, self._rows, params, x.shape[0], self._cols, x.device)
        return _run_pass(self._who, x, self.roi, self.fill, out, self._pass, params)

    def __call__(self, x: torch.Tensor, step: Optional[int] = None) -> torch.Tensor:
        """The augmented batch for this instance's running step (which then advances by one), or for `step` if given (the counter stays).
        The table used is kept in `last_params` (a device tensor; None for the identity)."""
        self._check_input(x)
        return _at_step(self._who, self, step, lambda step: self._augmented(x, step))

    def _augmented(self, x, step):
        if self.is_identity(x):
            self.last_params = None
            return x
        params = self.params(x.shape[0], step, in_size=tuple(x.shape[1:4]), device=x.device)
        out = self.apply(x, params)
        self.last_params = params
        return out


class VolumeAugment(_WindowTransform):
    """roi: (Sx, Sy, Sz) of the output window (an int = a cube).  Per sample and per axis: a crop offset uniform on [0, X - S] (monai's
    RandSpatialCrop with a fixed size), plus an integer translation uniform on [-max_shift, max_shift] (cells of the window that leave
    the volume get `fill`), a flip with probability flip_prob; per sample an intensity change x * scale + shift with scale / shift
    uniform on their (lo, hi) ranges.  The T timepoints of a 4D sample share its parameters.  Every option at its default switches that
    transform off; with the roi equal to the input size as well, the instance is the identity and `__call__` launches nothing.

    A row of `params` (int32 [B, 8]) is {ox, oy, oz, flip bits, bits of scale, bits of shift, 0, 0}.  seed, rank and the step index
    decide every draw (see nv_augment_params in the header): the same triple reproduces a batch, two ranks with one seed draw different
    parameters.  `step` counts the calls of this instance unless it is given."""
    _cols, _rows, _draw, _pass = 8, "params", "nv_augment_params", "nv_augment_apply"

    def __init__(self, roi, flip_prob=(0, 0, 0), max_shift=(0, 0, 0), scale=(1, 1), shift=(0, 0), fill: float = 0.0, seed: int = 0,
                 rank: int = 0):
        self._set_window(roi)
        self._set_flips(flip_prob)
        self.max_shift = _triple(self._who, max_shift, "max_shift", int)
        if any(m < 0 or m >= 2 ** 30 for m in self.max_shift):
            raise ValueError(f"{self._who}: max_shift must lie in [0, 2^30), got {self.max_shift}")
        self._set_shared(scale, shift, fill, seed, rank)

    def _transforms_off(self) -> bool:
        return self._shared_off() and all(m == 0 for m in self.max_shift)

    def _config(self, in_size):
        return AugmentConfig(ctypes.sizeof(AugmentConfig), (ctypes.c_int * 3)(*in_size), (ctypes.c_int * 3)(*self.roi),
                             (ctypes.c_int * 3)(*self.max_shift), (ctypes.c_double * 3)(*self.flip_prob), self.scale[0], self.scale[1],
                             self.shift[0], self.shift[1])


class AffineConfig(ctypes.Structure):
    """struct nv_affine_config (neurovit_hip.h, added within revision 8)."""
    _fields_ = [("struct_size", ctypes.c_int), ("in_size", ctypes.c_int * 3), ("roi", ctypes.c_int * 3), ("rotate_deg", ctypes.c_double * 3),
                ("zoom_lo", ctypes.c_double), ("zoom_hi", ctypes.c_double), ("isotropic", ctypes.c_int), ("translate", ctypes.c_double * 3),
                ("prob", ctypes.c_double), ("flip_prob", ctypes.c_double * 3), ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float),
                ("shift_lo", ctypes.c_float), ("shift_hi", ctypes.c_float)]


AFFINE_COLS = 16     # int32 columns of a row of nv_affine_params


class VolumeAffine(_WindowTransform):
    """Random rotation, zoom and sub-voxel translation on the device (monai's RandAffine / RandRotate / RandZoom), together with the crop,
    the flips and the intensity change of VolumeAugment, as ONE trilinear gather pass (nv_affine_apply).  roi: (Sx, Sy, Sz) of the output
    window (an int = a cube).  Per sample: a crop offset uniform on [0, X - S] per axis; with probability `prob` a rotation about the
    centre of the window by angles uniform on [-rotate, rotate] degrees about the x, y and z axes (composed Rz Ry Rx), a zoom uniform on
    `zoom` = (lo, hi) - one draw for the three axes when `isotropic`, one per axis otherwise; above 1 the content grows - and a
    translation uniform on [-translate, translate] voxels per axis; a flip per axis with probability flip_prob; an intensity change
    x * scale + shift.  Cells of the window whose source lies outside the volume blend towards `fill`.  The T timepoints of a 4D sample
    share its parameters.  Every option at its default switches that transform off; with the roi equal to the input size as well the
    instance is the identity and `__call__` launches nothing.  A sample that `prob` leaves out is the bit copy VolumeAugment would write.

    A row of `params` (int32 [B, 16]) is the fp32 bits of the 3 x 4 map output cell -> source coordinate (M_a0, M_a1, M_a2, m_a3 for
    a = x, y, z), the bits of scale and shift, flags (bits 0 .. 2 the flips, bit 3 "affine applied"), 0.  seed, rank and the step index
    decide every draw (nv_affine_params in the header; a hash domain of its own, so a VolumeAugment or VolumeMix with the same seed
    draws independently).  `step` counts the calls of this instance unless it is given."""
    _cols, _rows, _draw, _pass = AFFINE_COLS, "table", "nv_affine_params", "nv_affine_apply"

    def __init__(self, roi, rotate=0.0, zoom=(1, 1), isotropic: bool = True, translate=0.0, prob: float = 1.0, flip_prob=(0, 0, 0), scale=(1, 1),
                 shift=(0, 0), fill: float = 0.0, seed: int = 0, rank: int = 0):
        self._set_window(roi)
        self.rotate = _triple(self._who, rotate, "rotate", float)
        if any(not (abs(r) <= 180.0) for r in self.rotate):
            raise ValueError(f"{self._who}: rotate must lie in [-180, 180] degrees, got {self.rotate}")
        try:
            lo, hi = zoom
        except (TypeError, ValueError):
            raise TypeError(f"{self._who}: zoom must be a pair (lo, hi) of numbers, got {zoom!r}") from None
        if any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in (lo, hi)):
            raise TypeError(f"{self._who}: zoom must be a pair (lo, hi) of numbers, got {zoom!r}")
        if not (0.0 < lo <= hi <= 16.0):
            raise ValueError(f"{self._who}: zoom must satisfy 0 < lo <= hi <= 16, got {zoom!r}")
        self.zoom = (float(lo), float(hi))
        if not isinstance(isotropic, bool):
            raise TypeError(f"{self._who}: isotropic must be true or false, got {isotropic!r}")
        self.isotropic = isotropic
        self.translate = _triple(self._who, translate, "translate", float)
        if any(not (0.0 <= t < math.inf) for t in self.translate):
            raise ValueError(f"{self._who}: translate must be finite and not negative, got {self.translate}")
        if isinstance(prob, bool) or not isinstance(prob, (int, float)):
            raise TypeError(f"{self._who}: prob must be a number, got {prob!r}")
        if not (0.0 <= float(prob) <= 1.0):
            raise ValueError(f"{self._who}: prob {prob} outside [0, 1]")
        self.prob = float(prob)
        self._set_flips(flip_prob)
        self._set_shared(scale, shift, fill, seed, rank)

    def _transforms_off(self) -> bool:
        still = self.prob == 0.0 or (all(r == 0.0 for r in self.rotate) and self.zoom == (1.0, 1.0) and all(t == 0.0 for t in self.translate))
        return still and self._shared_off()

    def _config(self, in_size):
        return AffineConfig(ctypes.sizeof(AffineConfig), (ctypes.c_int * 3)(*in_size), (ctypes.c_int * 3)(*self.roi), (ctypes.c_double * 3)(*self.rotate),
                            self.zoom[0], self.zoom[1], int(self.isotropic), (ctypes.c_double * 3)(*self.translate), self.prob,
                            (ctypes.c_double * 3)(*self.flip_prob), self.scale[0], self.scale[1], self.shift[0], self.shift[1])


def center_window(x: torch.Tensor, roi: Sequence[int]) -> torch.Tensor:
    """The centre window of x [B, X, Y, Z(, T)] at offset (X - S) // 2 per axis, as a strided VIEW (x itself when the sizes agree)."""
    size = tuple(x.shape[1:4])
    if any(s > n for s, n in zip(roi, size)):
        raise ValueError(f"center_window: roi {tuple(roi)} is larger than the input {size}")
    if tuple(roi) == size:
        return x
    (ox, oy, oz) = ((n - s) // 2 for s, n in zip(roi, size))
    return x[:, ox:ox + roi[0], oy:oy + roi[1], oz:oz + roi[2]]


class MixConfig(ctypes.Structure):
    """struct nv_mix_config (neurovit_hip.h, added within revision 8)."""
    _fields_ = [("struct_size", ctypes.c_int), ("roi", ctypes.c_int * 3), ("mixup_alpha", ctypes.c_double), ("cutmix_alpha", ctypes.c_double),
                ("prob", ctypes.c_double), ("switch_prob", ctypes.c_double)]


class VolumeMix:
    """Mixup / CutMix on the device, per sample (timm's `elem` mode): sample b is paired with B - 1 - b (`flip(0)`), mixed with
    probability `prob`, by CutMix rather than Mixup with probability `switch_prob` when both alphas are set; lambda ~ Beta(alpha, alpha)
    with alpha in [0.05, 1].  Mixup writes lam * x + (1 - lam) * partner; CutMix pastes a box of the partner whose volume share is
    1 - lam before clipping (the label lambda is the share actually kept).  The T timepoints of a 4D sample share its row.  Both
    alphas None: the identity, nothing is launched.

    `params` draws the table on the device (nv_mix_params: int32 [B, 12] = {partner, mode, bits of the pixel lambda, bits of the label
    lambda, tries, x0, x1, y0, y1, z0, z1, 0}; the rule is in include/neurovit_hip.h and tests/mix_ref.py restates it); `apply` is ONE
    streaming launch (nv_augment_mix) that also does the work of a VolumeAugment when one is handed in - each sample and its partner
    under their own crop / flip / intensity rows - so that a batch is read and written once.  With a VolumeAffine it is TWO launches: the
    gather pass writes the dense window, the mix pass then runs on it with identity rows.  `last_mix` is what the loss needs
    (nn.CrossEntropyLoss.forward(..., mix=) / TrainStep.__call__(..., mix=)).  No gradient flows through it."""

    def __init__(self, mixup_alpha: Optional[float] = None, cutmix_alpha: Optional[float] = None, prob: float = 1.0, switch_prob: float = 0.5,
                 seed: int = 0, rank: int = 0):
        for name, a in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if a is None:
                continue
            if isinstance(a, bool) or not isinstance(a, (int, float)):
                raise TypeError(f"VolumeMix: {name} must be a number or None, got {a!r}")
            if not (0.05 <= float(a) <= 1.0):
                raise ValueError(f"VolumeMix: {name} {a} outside [0.05, 1] (the Beta sampler's range)")
        for name, p in (("prob", prob), ("switch_prob", switch_prob)):
            if isinstance(p, bool) or not isinstance(p, (int, float)):
                raise TypeError(f"VolumeMix: {name} must be a number, got {p!r}")
            if not (0.0 <= float(p) <= 1.0):
                raise ValueError(f"VolumeMix: {name} {p} outside [0, 1]")
        _check_seed_rank("VolumeMix", seed, rank)
        self.mixup_alpha = None if mixup_alpha is None else float(mixup_alpha)
        self.cutmix_alpha = None if cutmix_alpha is None else float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.seed, self.rank = seed, rank
        self.step = 0                      # the step index the next __call__ without `step=` draws for
        self.last_mix: Optional[torch.Tensor] = None

    def is_identity(self) -> bool:
        return self.mixup_alpha is None and self.cutmix_alpha is None

    @staticmethod
    def _check_input(x: torch.Tensor):
        _check_volume("VolumeMix", "mix", x)

    def params(self, B: int, step: int, roi, device=None) -> torch.Tensor:
        """int32 [B, 12] on the device for step `step`; roi: (Sx, Sy, Sz) of the batch that will be mixed (the CutMix box lives in it)."""
        step = _check_step("VolumeMix", step)
        roi = _triple("VolumeMix", roi, "roi", int)
        if any(s <= 0 for s in roi):
            raise ValueError(f"VolumeMix: roi must be positive, got {roi}")
        device = _draw_target("VolumeMix", B, device)
        out = torch.empty((B, MIX_COLS), dtype=torch.int32, device=device)
        cfg = MixConfig(ctypes.sizeof(MixConfig), (ctypes.c_int * 3)(*roi), self.mixup_alpha or 0.0, self.cutmix_alpha or 0.0, self.prob, self.switch_prob)
        with torch.cuda.device(device):
            check(lib.nv_mix_params(ctypes.byref(cfg), self.seed, step, self.rank, B, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "nv_mix_params")
        return out

    def apply(self, x: torch.Tensor, mix: torch.Tensor, augment: Union[VolumeAugment, VolumeAffine, None] = None,
              augment_params: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B, X, Y, Z(, T)] float32 on the device, dense or a strided view; mix int32 [B, 12].  With `augment` (a VolumeAugment: its
        roi and fill) and `augment_params` (int32 [B, 8], its rows) the crop / flips / intensity change happen in the same pass; without,
        the window is the whole volume and every row the identity.  With a VolumeAffine and its table (int32 [B, 16]) the gather pass
        runs first and the mix pass on its dense output: two launches.  Returns the dense [B, Sx, Sy, Sz(, T)] batch."""
        if augment is not None and not isinstance(augment, (VolumeAugment, VolumeAffine)):
            raise TypeError(f"VolumeMix.apply: augment must be a VolumeAugment or a VolumeAffine, got {type(augment).__name__}")
        if (augment is None) != (augment_params is None):
            raise ValueError("VolumeMix.apply: augment and augment_params come together")
        if isinstance(augment, VolumeAffine):
            window = augment.apply(x, augment_params)
            mix = _check_rows("VolumeMix", "mix", mix, x.shape[0], MIX_COLS, x.device)
            return _run_pass("VolumeMix", window, augment.roi, 0.0, out, "nv_augment_mix", None, mix)
        roi = None if augment is None else augment.roi
        _check_volume("VolumeMix", "mix", x, roi)
        B = x.shape[0]
        mix = _check_rows("VolumeMix", "mix", mix, B, MIX_COLS, x.device)
        if augment_params is not None:
            augment_params = _check_rows("VolumeMix", "augment_params", augment_params, B, 8, x.device)
        return _run_pass("VolumeMix", x, roi or tuple(x.shape[1:4]), 0.0 if augment is None else augment.fill, out, "nv_augment_mix", augment_params, mix)

    def __call__(self, x: torch.Tensor, step: Optional[int] = None, augment: Union[VolumeAugment, VolumeAffine, None] = None) -> torch.Tensor:
        """The mixed batch for this instance's running step (which then advances by one), or for `step` if given (the counter stays).
        augment: a VolumeAugment to apply in the same pass - or a VolumeAffine, whose gather pass runs in front of the mix pass - with ITS
        draws for the same step index (its last_params is set; its own counter is not touched).  The table used is kept in `last_mix`
        (a device tensor; None for the identity)."""
        if augment is not None and not isinstance(augment, (VolumeAugment, VolumeAffine)):
            raise TypeError(f"VolumeMix: augment must be a VolumeAugment or a VolumeAffine, got {type(augment).__name__}")
        return _at_step("VolumeMix", self, step, lambda step: self._mixed(x, step, augment))

    def _mixed(self, x, step, augment):
        self._check_input(x)
        if self.is_identity():
            self.last_mix = None
            return x if augment is None else augment(x, step=step)
        B = x.shape[0]
        if augment is None or augment.is_identity(x):
            aug, rows, roi = None, None, tuple(x.shape[1:4])
            if augment is not None:
                augment._check_input(x)
                augment.last_params = None
        else:
            augment._check_input(x)
            aug, roi = augment, augment.roi
            rows = augment.last_params = augment.params(B, step, in_size=tuple(x.shape[1:4]), device=x.device)
        mix = self.params(B, step, roi, device=x.device)
        out = self.apply(x, mix, augment=aug, augment_params=rows)
        self.last_mix = mix
        return out
