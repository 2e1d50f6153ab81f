"""ctypes binding of libneurovit_hip.so (the gfx950 C-ABI, include/neurovit_hip.h).

The prototypes are parsed from the header itself so the binding cannot drift from it.
There is NO fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "neurovit_hip.h")
# NEUROVIT_HIP_LIB: another build of the same library (same-box A/B runs of two builds in one gpurun call: tools/_ab/); the tree's own otherwise
LIB_PATH = os.environ.get("NEUROVIT_HIP_LIB") or os.path.join(_HERE, "lib", "libneurovit_hip.so")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}


class VitConfig(ctypes.Structure):
    """struct nv_vit_config (neurovit_hip.h) == ctor arguments of the reference ViT (vit_3d.py:78)."""
    _fields_ = [("image_size", ctypes.c_int), ("image_patch_size", ctypes.c_int), ("frames", ctypes.c_int),
                ("frame_patch_size", ctypes.c_int), ("channels", ctypes.c_int), ("num_classes", ctypes.c_int),
                ("dim", ctypes.c_int), ("depth", ctypes.c_int), ("heads", ctypes.c_int), ("dim_head", ctypes.c_int),
                ("mlp_dim", ctypes.c_int), ("ln_eps", ctypes.c_float), ("pool_mean", ctypes.c_int),
                ("image_width", ctypes.c_int), ("patch_width", ctypes.c_int),      # 0 = square
                ("no_proj_dropout", ctypes.c_int)]      # heads == 1 and dim_head == dim: to_out is nn.Identity(), no Dropout behind it (vit_3d.py:43-46)


class VitInput(ctypes.Structure):
    """struct nv_vit_input (neurovit_hip.h): optional input forms of nv_vit_forward_in / nv_vit_forward_fp8, and (revision 8) the
    attention-probability export (a pointer to an AttnExport, or None)."""
    _fields_ = [("vol_sigma", ctypes.c_void_p), ("time_points", ctypes.c_int), ("rows_form", ctypes.c_int), ("attn_export", ctypes.c_void_p)]


class AttnExport(ctypes.Structure):
    """struct nv_vit_attn_export (neurovit_hip.h, revision 8): per-layer output pointers (a HOST array, NULL = layer not exported),
    the head fusion (ATTN_FUSIONS) and the rows (ATTN_ROWS) of the probabilities a forward writes behind each attention launch."""
    _fields_ = [("struct_size", ctypes.c_int), ("maps", ctypes.c_void_p), ("fusion", ctypes.c_int), ("rows", ctypes.c_int)]


ATTN_FUSIONS = {None: 0, "mean": 1, "max": 2, "min": 3}     # NV_ATTN_PER_HEAD, NV_ATTN_FUSE_MEAN / _MAX / _MIN
ATTN_ROWS = {"all": 0, "cls": 1}                            # NV_ATTN_ROWS_ALL / NV_ATTN_ROWS_CLS


class AttnGradExport(ctypes.Structure):
    """struct nv_vit_attn_grad_export (neurovit_hip.h, added within revision 8): per-layer output pointers (a HOST array, NULL = layer not
    exported) and the form (ATTN_GRAD_FORMS) of the attention gradients nv_vit_backward_attn writes behind each attention backward."""
    _fields_ = [("struct_size", ctypes.c_int), ("maps", ctypes.c_void_p), ("form", ctypes.c_int)]


ATTN_GRAD_FORMS = {"per_head": 0, "relevance": 1}           # NV_ATTN_GRAD_PER_HEAD / NV_ATTN_GRAD_RELEVANCE


class TrainHparams(ctypes.Structure):
    """struct nv_train_hparams (neurovit_hip.h): optimizer constants and accumulation flags of nv_vit_train_step."""
    _fields_ = [("struct_size", ctypes.c_int), ("step", ctypes.c_int), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("grad_scale", ctypes.c_float),
                ("accumulate", ctypes.c_int), ("update", ctypes.c_int), ("fuse_update", ctypes.c_int),
                ("loss_scale", ctypes.c_float), ("dp", ctypes.c_void_p), ("loss_scale_state", ctypes.c_void_p)]


class DpPlan(ctypes.Structure):
    """struct nv_dp_plan (neurovit_hip.h): the data-parallel form of nv_vit_train_step's backward pass + update."""
    _fields_ = [("struct_size", ctypes.c_int), ("world", ctypes.c_int), ("comm", ctypes.c_void_p), ("comm_stream", ctypes.c_void_p),
                ("n_buckets", ctypes.c_int), ("update_per_bucket", ctypes.c_int), ("grads16", ctypes.c_void_p)]


class AdamwArena(ctypes.Structure):
    """struct nv_adamw_arena (neurovit_hip.h): AdamW constants + the five arenas that share element offsets."""
    _fields_ = [("struct_size", ctypes.c_int), ("step", ctypes.c_int), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("grad_scale", ctypes.c_float),
                ("keep_grads", ctypes.c_int), ("params", ctypes.c_void_p), ("grads", ctypes.c_void_p), ("adam_m", ctypes.c_void_p),
                ("adam_v", ctypes.c_void_p), ("params16", ctypes.c_void_p)]


class BackwardOpts(ctypes.Structure):
    """struct nv_vit_backward_opts (neurovit_hip.h, revision 7): options of nv_vit_backward_ex - the gradient w.r.t. the input volume
    (dvideo + its element strides) and the data-only backward (weight_grads = 0)."""
    _fields_ = [("struct_size", ctypes.c_int), ("dvideo", ctypes.c_void_p), ("dvideo_strides5", ctypes.c_void_p), ("weight_grads", ctypes.c_int)]


class LossOpts(ctypes.Structure):
    """struct nv_loss_opts (neurovit_hip.h, added within revision 8): label smoothing, class weights and the mix table of the
    soft-target cross-entropy (nv_ce_loss_soft / nv_head_step_soft / nv_vit_train_step_ex)."""
    _fields_ = [("struct_size", ctypes.c_int), ("label_smoothing", ctypes.c_float), ("class_weight", ctypes.c_void_p), ("mix", ctypes.c_void_p)]


class DropPath(ctypes.Structure):
    """struct nv_vit_drop_path (neurovit_hip.h, added within revision 8): the device table of stochastic-depth factors [depth][2][B] of
    nv_vit_forward_sd / nv_vit_backward_sd / nv_vit_train_step_sd."""
    _fields_ = [("struct_size", ctypes.c_int), ("factors", ctypes.c_void_p)]


class RegOpts(ctypes.Structure):
    """struct nv_reg_opts (neurovit_hip.h, added within revision 8): kind, huber's delta, the targets' mean / std, per-target weights and the
    mix table of the regression loss (nv_reg_loss / nv_head_step_reg / nv_vit_train_step_reg)."""
    _fields_ = [("struct_size", ctypes.c_int), ("kind", ctypes.c_int), ("delta", ctypes.c_float), ("mean", ctypes.c_void_p), ("std", ctypes.c_void_p),
                ("weight", ctypes.c_void_p), ("mix", ctypes.c_void_p)]


REG_KINDS = {"mse": 0, "l1": 1, "huber": 2}                 # NV_REG_MSE / NV_REG_L1 / NV_REG_HUBER
REG_METRIC_SLOTS = 9                                        # NV_REG_METRIC_SLOTS: doubles per target of the metrics' state
REG_METRIC_NAMES = ("n", "mae", "rmse", "bias", "r", "r2")  # the columns nv_reg_metrics_finish writes


CLS_KINDS = {"logits": 0, "probs": 1}                       # NV_CLS_LOGITS / NV_CLS_PROBS
CLS_MAX_C, CLS_MAX_BINS, CLS_STATE_HEAD = 64, 64, 6         # NV_CLS_MAX_C, NV_CLS_MAX_BINS, NV_CLS_STATE_HEAD (doubles in front of the confusion matrix)
CLS_STATE_NAMES = ("n", "skipped", "nll_sum", "batch_mean_sum", "batches", "brier_sum")      # the head of nv_cls_metrics_update's state
CLS_METRIC_NAMES = ("n", "skipped", "accuracy", "balanced_accuracy", "macro_f1", "nll", "val_loss", "brier", "ece", "macro_auc")   # NV_CLS_SCALARS
CLS_CLASS_METRIC_NAMES = ("support", "recall", "precision", "f1", "auc")                     # NV_CLS_CLASS_COLS: the per-class columns of the table
CLS_AUC_NAMES = ("auc", "n_pos", "n_neg", "gt", "eq")       # NV_CLS_AUC_COLS: the columns of nv_cls_auc's double table
CLS_AUC_MAX_N, CLS_AUC_MAX_SPLITS = 1 << 20, 256            # NV_CLS_AUC_MAX_N, NV_CLS_AUC_MAX_SPLITS


PERM_KINDS = {"one_sample": 0, "two_sample": 1}             # NV_PERM_ONE_SAMPLE / NV_PERM_TWO_SAMPLE
PERM_TAILS = {"two": 0, "greater": 1, "less": 2}            # NV_PERM_TAIL_TWO / _GREATER / _LESS
PERM_MAX_N, PERM_MAX_R, PERM_MAX_SPLITS, PERM_MAX_ALPHAS = 256, 1 << 20, 256, 8      # NV_PERM_MAX_N, NV_PERM_MAX_R, NV_PERM_MAX_SPLITS, NV_PERM_MAX_ALPHAS
PERM_TILE_V, PERM_TILE_R = 64, 64                           # NV_PERM_TILE_V, NV_PERM_TILE_R: voxels and rows of one tile of nv_perm_maxstat


POOL_MODES = {"cls": 0, "mean": 1, "patch_mean": 2}         # NV_POOL_CLS / NV_POOL_MEAN / NV_POOL_PATCH_MEAN
KNN_WEIGHTS = {"uniform": 0, "softmax": 1}                  # NV_KNN_UNIFORM / NV_KNN_SOFTMAX
KNN_MAX_K = 128                                             # NV_KNN_MAX_K


PROBE_CHUNK, PROBE_MAX_M, PROBE_MAX_D = 256, 32, 1024     # NV_PROBE_CHUNK, NV_PROBE_MAX_M, NV_PROBE_MAX_D
PROBE_TASKS = {"classification": 0, "regression": 1}        # NV_PROBE_CLASSIFICATION / NV_PROBE_REGRESSION


class ProbeHeads(ctypes.Structure):
    """struct nv_probe_heads (neurovit_hip.h, added within revision 8): the heads of a linear probe - H heads of C columns, the L2 strength per
    head (nv_probe_grad) and the Adam step size lr / (1 - beta1^t) per head (nv_probe_step)."""
    _fields_ = [("struct_size", ctypes.c_int), ("H", ctypes.c_int), ("C", ctypes.c_int), ("l2", ctypes.c_float * PROBE_MAX_M),
                ("step", ctypes.c_float * PROBE_MAX_M)]


DROP_PATH_SCHEDULES = {"linear": 0, "constant": 1}          # NV_DROP_PATH_LINEAR / NV_DROP_PATH_CONSTANT


ADAMW_MAX_GROUPS, ADAMW_MAX_SEGMENTS = 64, 1024      # NV_ADAMW_MAX_GROUPS, NV_ADAMW_MAX_SEGMENTS


class AdamwGroups(ctypes.Structure):
    """struct nv_adamw_groups (neurovit_hip.h, added within revision 8): the per-call half of nv_adamw_step_grouped's table - lr and
    weight_decay per group - and the device address of the segment table that nv_adamw_segments_build filled."""
    _fields_ = [("struct_size", ctypes.c_int), ("n_groups", ctypes.c_int), ("segments", ctypes.c_void_p),
                ("lr", ctypes.c_double * ADAMW_MAX_GROUPS), ("weight_decay", ctypes.c_double * ADAMW_MAX_GROUPS)]


MIX_COLS = 12        # NV_MIX_COLS: int32 columns of a row of nv_mix_params


ABI_VERSION = 8      # NV_ABI_VERSION of the header this binding was written against (checked at load time)


def parse_header(path: str = HEADER) -> Dict[str, Tuple[object, List[object]]]:
    """{symbol: (restype, [argtypes])} for every `nv_*` prototype declared in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int|long|const char\s*\*)\s+(nv_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        restype = ctypes.c_char_p if "char" in ret else _SCALARS[ret]
        argtypes = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(ctypes.c_char_p if re.match(r"const char\s*\*", a) else ctypes.c_void_p)
                elif a.startswith("unsigned long"):
                    argtypes.append(ctypes.c_ulong)
                else:
                    argtypes.append(_SCALARS[a.split()[0]])
        protos[name] = (restype, argtypes)
    return protos


class _Lib:
    def __init__(self):
        self._dll = None
        self.protos = parse_header()

    def load(self):
        if self._dll is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"neurovit_amd: {LIB_PATH} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or `make -C neurovit_amd/csrc`). There is no CPU / PyTorch fallback for this path.")
            dll = ctypes.CDLL(LIB_PATH)
            for name, (restype, argtypes) in self.protos.items():
                fn = getattr(dll, name)          # AttributeError if the .so lacks a declared symbol
                fn.restype, fn.argtypes = restype, argtypes
            got = dll.nv_abi_version()
            if got != ABI_VERSION:
                raise RuntimeError(f"neurovit_amd: {LIB_PATH} has ABI revision {got}, this binding expects {ABI_VERSION} - rebuild the library "
                                   "(make -C neurovit_amd/csrc); see INTEGRATION.md 'ABI revisions'")
            if os.environ.get("NEUROVIT_ATTN_MODE"):           # A/B aid: nv_attn_set_mode for the whole process (see the header)
                dll.nv_attn_set_mode(int(os.environ["NEUROVIT_ATTN_MODE"]))
            if os.environ.get("NEUROVIT_ADAMW_WGS"):           # A/B aid: workgroups of the weight-gradient launch with the AdamW epilogue
                dll.nv_gemm_set_tile(12, int(os.environ["NEUROVIT_ADAMW_WGS"]))
            if os.environ.get("NEUROVIT_HEAD_STEP"):           # A/B aid: 0 = the native step runs the head as three calls
                dll.nv_vit_set_head_step(int(os.environ["NEUROVIT_HEAD_STEP"]))
            if os.environ.get("NEUROVIT_WGRAD_WGS"):           # A/B aid: workgroups of the grouped weight-gradient launch
                dll.nv_gemm_set_tile(14, int(os.environ["NEUROVIT_WGRAD_WGS"]))
            if os.environ.get("NEUROVIT_PATCH_MODE"):          # A/B aid: 2 = the LDS-staged slab form of the patch gather instead of the per-token one
                dll.nv_patch_set_mode(int(os.environ["NEUROVIT_PATCH_MODE"]))
            if os.environ.get("NEUROVIT_ADAMW_CAP"):
                dll.nv_gemm_set_tile(13, int(os.environ["NEUROVIT_ADAMW_CAP"]))
            self._dll = dll
        return self._dll

    def __getattr__(self, name):
        return getattr(self.load(), name)


lib = _Lib()


OPERAND_FORMATS = {"bf16": 0, "fp16": 1}      # NV_OPERAND_BF16 / NV_OPERAND_FP16
_operand_format = "bf16"                      # what the library is set to (its own default)


def set_operand_format(fmt: str) -> None:
    """Select what every 16-bit buffer of the following calls holds and which MFMA contracts it (nv_set_operand_format): "bf16" (default)
    or "fp16" - the reference's autocast arithmetic (src/Trainer.py:68).  Process-wide in the library; modules set their own format
    in front of their calls, so models of both formats can live in one process.  Costs a C call only when the format changes."""
    global _operand_format
    if fmt != _operand_format:
        if fmt not in OPERAND_FORMATS:
            raise ValueError(f"neurovit_amd: operand format must be 'bf16' or 'fp16', got {fmt!r}")
        check(lib.nv_set_operand_format(OPERAND_FORMATS[fmt]), "nv_set_operand_format")
        _operand_format = fmt


def operand_format() -> str:
    return _operand_format


def last_error() -> str:
    return (lib.nv_last_error() or b"").decode()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise RuntimeError(f"neurovit_amd C-ABI call failed ({what}, rc={rc}): {last_error()}")


def require_gpu() -> None:
    """Fail loudly unless a gfx950 device and the HIP library are usable."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("neurovit_amd: no HIP device available - this path only runs on MI355X (gfx950); "
                           "there is no CPU fallback.")
    if lib.nv_arch_ok() != 1:
        raise RuntimeError(f"neurovit_amd: current device is not gfx950: {last_error()}")
