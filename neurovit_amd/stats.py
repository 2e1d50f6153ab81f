"""Group-level permutation tests with the maximum statistic over attribution maps (csrc/perm_test.hip: nv_perm_design / nv_perm_stats /
nv_perm_maxstat / nv_perm_finish).

    maps = attribution_volumes(...)                       # [N, S, S, S], one per volume, on the device
    res = permutation_test(maps, subjects=subject_ids)    # one sample: where is the attribution consistently non-zero across subjects?
    region = res["p_fwe"] < 0.05                          # family-wise error controlled over all voxels (Nichols & Holmes)

    res = permutation_test(maps, labels=patient, subjects=subject_ids)      # two samples: where do patients (1) and controls (0) differ?

labels=None: the one-sample test by sign flips (H0: the maps are symmetric about 0).  labels of 0 / 1: the two-sample pooled-variance Student
t under label permutation; t > 0 where group 1 has the larger mean.  A PAIRED design is the one-sample test on the differences: pass
maps_a - maps_b.  For N subjects with 2^N <= permutations (the 17-subject validation cohort: 131 072 rows) every sign flip is enumerated and
the p-values are exact.  The product of the design with the maps is never written: one fp32 MFMA kernel reduces it to the row maxima and the
per-voxel exceedance counts.  PyTorch owns the buffers; there is no CPU fallback and no host read inside the call."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import torch

from . import _cabi
from ._cabi import check, lib
from .ops import Segments, _p, _rows2d, _stream, host_ids


def perm_workspace(R: int, V: int, splits: int = 0, device="cuda") -> torch.Tensor:
    """the workspace one test's perm_stats / perm_maxstat / perm_finish calls share (nv_perm_workspace_bytes)"""
    need = int(lib.nv_perm_workspace_bytes(int(R), int(V), int(splits)))
    if need <= 0:
        raise ValueError(f"permutation test: R = {R} outside [1, {_cabi.PERM_MAX_R}], V = {V} not positive or splits = {splits} outside [0, {_cabi.PERM_MAX_SPLITS}]")
    return torch.empty(need, dtype=torch.uint8, device=device)


def perm_design(kind: str, N: int, R: int, *, labels: Optional[torch.Tensor] = None, n_a: int = 0, exact: bool = False, seed: int = 0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nv_perm_design: the design matrix fp32 [R, Npad] (Npad = N rounded up to 4); labels: device int32 [N] of 0 / 1 with n_a ones (two samples)"""
    Npad = (N + 3) & ~3
    if out is None:
        out = torch.empty((max(int(R), 1), Npad), dtype=torch.float32, device="cuda")
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= max(int(R), 1) * Npad
    check(lib.nv_perm_design(_cabi.PERM_KINDS[kind], int(N), int(n_a), _p(labels), int(R), 1 if exact else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(out), _stream()),
          "nv_perm_design")
    return out


def perm_stats(X: torch.Tensor, kind: str, workspace: torch.Tensor, *, labels: Optional[torch.Tensor] = None, n_a: int = 0,
               mask: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """nv_perm_stats: {"a", "c", "t": fp32 [V], "n_invalid": int32 [1]} of the maps X fp32 [N, V] (a row-strided view passes its leading dimension)"""
    N, V = _rows2d(X, "perm_stats: X")
    out = out or {}
    for key in ("a", "c", "t"):
        out.setdefault(key, torch.empty(V, dtype=torch.float32, device=X.device))
    out.setdefault("n_invalid", torch.empty(1, dtype=torch.int32, device=X.device))
    if mask is not None:
        assert mask.is_cuda and mask.dtype in (torch.bool, torch.uint8) and mask.numel() == V and mask.is_contiguous()
    check(lib.nv_perm_stats(_p(X), X.stride(0), N, V, _cabi.PERM_KINDS[kind], int(n_a), _p(labels), _p(mask), _p(out["a"]), _p(out["c"]), _p(out["t"]),
                            _p(out["n_invalid"]), _p(workspace), workspace.numel(), _stream()), "nv_perm_stats")
    return out


def perm_maxstat(X: torch.Tensor, M: torch.Tensor, a: torch.Tensor, c: torch.Tensor, workspace: torch.Tensor, *, tail: str = "two", splits: int = 0) -> None:
    """nv_perm_maxstat: the fused product + reduction of all R rows of M against the maps; the partials stay in the workspace for perm_finish"""
    N, V = _rows2d(X, "perm_maxstat: X")
    R = M.shape[0]
    check(lib.nv_perm_maxstat(_p(X), X.stride(0), N, V, _p(M), R, _p(a), _p(c), _cabi.PERM_TAILS[tail], int(splits), _p(workspace), workspace.numel(), _stream()),
          "nv_perm_maxstat")


def perm_finish(kind: str, N: int, R: int, V: int, c: torch.Tensor, workspace: torch.Tensor, *, alphas: Sequence[float] = (), splits: int = 0,
                out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """nv_perm_finish: {"max_stat", "max_t": fp32 [R], "count_unc", "count_fwe": int32 [V], "p_unc", "p_fwe": fp32 [V], "critical_t": fp32 [len(alphas)]}"""
    out = out or {}
    dev = c.device
    for key in ("max_stat", "max_t"):
        out.setdefault(key, torch.empty(R, dtype=torch.float32, device=dev))
    for key in ("count_unc", "count_fwe"):
        out.setdefault(key, torch.empty(V, dtype=torch.int32, device=dev))
    for key in ("p_unc", "p_fwe"):
        out.setdefault(key, torch.empty(V, dtype=torch.float32, device=dev))
    out.setdefault("critical_t", torch.empty(len(alphas), dtype=torch.float32, device=dev))
    al = (ctypes.c_double * max(len(alphas), 1))(*[float(x) for x in alphas])
    check(lib.nv_perm_finish(_cabi.PERM_KINDS[kind], int(N), int(R), int(V), int(splits), _p(c), ctypes.cast(al, ctypes.c_void_p), len(alphas), _p(out["max_stat"]),
                             _p(out["max_t"]), _p(out["count_unc"]), _p(out["count_fwe"]), _p(out["p_unc"]), _p(out["p_fwe"]),
                             _p(out["critical_t"]) if len(alphas) else None, _p(workspace), workspace.numel(), _stream()), "nv_perm_finish")
    return out


def _host_labels(labels, n: int) -> torch.Tensor:
    """0 / 1 labels [n] as an int32 HOST tensor.  They are host data, as subject ids are: the group sizes, and with `subjects` the label of
    each subject, are settled on the host, so that the call reads nothing back from the device."""
    if torch.is_tensor(labels) and labels.is_cuda:
        raise ValueError("permutation_test: labels are host data (a sequence, an array or a CPU tensor) - a device tensor would cost a read-back")
    lab = torch.as_tensor(labels)
    lab = host_ids(lab.to(torch.int32) if lab.dtype == torch.bool else lab, n, "permutation_test: labels of 0 / 1")
    if not bool(((lab == 0) | (lab == 1)).all()):
        raise ValueError("permutation_test: labels must be 0 or 1")
    return lab


def permutation_test(maps: torch.Tensor, labels=None, permutations: int = 10000, tail: str = "two", mask: Optional[torch.Tensor] = None, subjects=None,
                     seed: int = 0, exact: Optional[bool] = None, alphas: Sequence[float] = (0.05, 0.01), splits: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Voxel-wise permutation test of maps fp32 [N, ...] on the device (the output of attribution_volumes, token_maps, occlusion_sensitivity or
    shapley_values(...)["token_maps"] as it is) with uncorrected and max-statistic FWE-corrected p-values.

    labels     None: one sample, sign flips.  0 / 1 per row (host data): two samples, label permutation, Student t with pooled variance.
               A paired design is the one-sample test on the differences of the pairs.
    permutations  rows of the design, the observed labelling included as row 0 (p >= 1 / rows); at most 2^20.
    tail       "two" (|t|), "greater" or "less".
    mask       bool [...] on the device: voxels outside it are not tested (NaN) and enter no maximum.
    subjects   host ids per row (as FeatureBank takes them; GroupIndex makes them): rows are averaged per subject first (nv_segment_mean) and
               the subjects are the units that are flipped or permuted.  A subject's label is that of its first row; mixed labels are refused.
    exact      one sample only.  None: enumerate all 2^N sign flips when 2^N <= permutations; True: enumerate (refused for N > 20).
    alphas     family-wise levels of the critical values.
    splits     row splits of the hot kernel (None = automatic); no output bit depends on it.

    Returns device tensors: "t" (observed statistic), "p_unc", "p_fwe" (all of the maps' trailing shape; NaN in an invalid voxel - outside the
    mask, a non-finite value, zero variance), "max_t" [rows] (the null distribution of the maximum, in t units), "critical_t" [len(alphas)],
    "n_permutations" (the rows), "n_invalid", "exact"."""
    if not torch.is_tensor(maps) or maps.dtype != torch.float32 or maps.dim() < 2:
        raise ValueError("permutation_test: maps must be a float32 tensor [N, ...]")
    if tail not in _cabi.PERM_TAILS:
        raise ValueError(f"permutation_test: tail must be 'two', 'greater' or 'less', got {tail!r}")
    alphas = [float(x) for x in alphas]
    if len(alphas) > _cabi.PERM_MAX_ALPHAS or any(not 0.0 < x < 1.0 for x in alphas):
        raise ValueError(f"permutation_test: at most {_cabi.PERM_MAX_ALPHAS} alphas, each inside (0, 1), got {alphas}")
    S = 0 if splits is None else int(splits)
    if S < 0 or S > _cabi.PERM_MAX_SPLITS:
        raise ValueError(f"permutation_test: splits = {splits} outside [0, {_cabi.PERM_MAX_SPLITS}]")
    rows, shape = maps.shape[0], tuple(maps.shape[1:])
    V = 1
    for s in shape:
        V *= int(s)
    if V < 1:
        raise ValueError("permutation_test: the maps are empty")
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != shape):
        raise ValueError(f"permutation_test: mask must be a bool tensor of shape {shape}")
    lab = None if labels is None else _host_labels(labels, rows)
    N = rows
    if subjects is not None:
        subjects = Segments(host_ids(subjects, rows, "permutation_test subjects"))      # (no row in a subject: refused there)
        N = subjects.G
        if bool((subjects.sizes == 0).any()):
            raise ValueError("permutation_test: subject ids must be dense (0 .. G - 1, each with a row); GroupIndex makes such ids")
        if lab is not None:
            lab, mixed = subjects.host_first_labels(lab)
            if mixed:
                raise ValueError("permutation_test: mixed labels - the rows of a subject carry different labels")
    kind = "one_sample" if lab is None else "two_sample"
    n_a = 0 if lab is None else int((lab == 1).sum())
    if N < 2 or N > _cabi.PERM_MAX_N:
        raise ValueError(f"permutation_test: {N} subjects outside [2, {_cabi.PERM_MAX_N}]")
    if kind == "two_sample" and (N < 3 or n_a < 1 or n_a > N - 1):
        raise ValueError(f"permutation_test: two samples need at least 3 subjects and both groups non-empty, got N = {N} with {n_a} of label 1")
    if kind == "two_sample" and exact:
        raise ValueError("permutation_test: exact enumeration exists for the one-sample test only")
    if exact and N > 20:
        raise ValueError(f"permutation_test: exact enumeration of 2^{N} sign flips exceeds the {_cabi.PERM_MAX_R} rows of a call")
    permutations = int(permutations)
    enumerate_all = kind == "one_sample" and (bool(exact) or (exact is None and N <= 20 and (1 << N) <= permutations))
    R = (1 << N) if enumerate_all else permutations
    if R < 1 or R > _cabi.PERM_MAX_R:
        raise ValueError(f"permutation_test: permutations = {R} outside [1, {_cabi.PERM_MAX_R}]")
    if not maps.is_cuda or (mask is not None and not mask.is_cuda):
        raise RuntimeError("permutation_test runs on the MI355X only (got a CPU tensor); there is no CPU fallback")
    dev = maps.device
    X = maps.reshape(rows, V)
    if X.stride(1) != 1:
        X = X.contiguous()
    if subjects is not None:
        X = subjects.mean(X)
    lab_dev = None if lab is None else lab.to(dev)
    mask_dev = None if mask is None else mask.reshape(V).contiguous()
    ws = perm_workspace(R, V, S, dev)
    M = perm_design(kind, N, R, labels=lab_dev, n_a=n_a, exact=enumerate_all, seed=seed)
    st = perm_stats(X, kind, ws, labels=lab_dev, n_a=n_a, mask=mask_dev)
    perm_maxstat(X, M, st["a"], st["c"], ws, tail=tail, splits=S)
    fin = perm_finish(kind, N, R, V, st["c"], ws, alphas=alphas, splits=S)
    return {"t": st["t"].reshape(shape), "p_unc": fin["p_unc"].reshape(shape), "p_fwe": fin["p_fwe"].reshape(shape), "max_t": fin["max_t"],
            "critical_t": fin["critical_t"], "n_permutations": torch.full((), R, dtype=torch.int32, device=dev), "n_invalid": st["n_invalid"].reshape(()),
            "exact": torch.full((), enumerate_all, dtype=torch.bool, device=dev)}
