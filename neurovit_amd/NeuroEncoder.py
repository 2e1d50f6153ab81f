"""Drop-in for the reference's src/models/NeuroEncoder.py on MI355X.

Same classes / constructor signatures / forward signatures / state_dict keys / attribute paths
(NeuroEncoder.py:15-230): NeuroEncoder(config), ViT3DEncoder(config), TemporalTransformer(config),
ProjectionHead(config); `model.activations`, `model.gradients`, `get_attention_map`, `visualize_slice`.

Config: the reference hard-codes dim=1024, depth=6, heads=8, mlp_dim=2048 (NeuroEncoder.py:181-195).
Optional keys TRAINING_VIT_DIM / _DEPTH / _HEADS / _DIM_HEAD / _MLP_DIM override them and default to
those constants, so an unmodified configs/config.yaml builds the same model.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .vit_3d import ViT, cached_table, target_classes


def _encoder_weights_of(checkpoint: dict, prefix: str = "volume_encoder.") -> dict:
    """The entries of a 3D NeuroEncoder checkpoint that belong to its ViT3DEncoder, re-keyed for that sub-module: the 4D model is
    built around the encoder of a trained 3D model (NeuroEncoder.py:23-31) and nothing else of that file is used."""
    wanted = prefix + "vit3d."
    return {key[len(prefix):]: tensor for key, tensor in checkpoint.items() if key.startswith(wanted)}


def perturbation_step_bounds(tokens: int, steps: int, device=None) -> torch.Tensor:
    """int64 [steps + 1]: m_k = (2 k N + steps) // (2 steps), the number of top-ranked patches point k of a deletion / insertion curve has
    removed / present - k N / steps rounded half up in integers, so m_0 = 0, m_steps = N and the bounds never decrease."""
    k = torch.arange(steps + 1, device=device, dtype=torch.int64)
    return (2 * k * tokens + steps) // (2 * steps)


def _grid_geometry(config, threshold=None):
    """(size S of the volume, cells G per axis of its patch grid, percent of the cells a map keeps: `threshold`, None = GRADCAM_THRESHOLD)"""
    size = config['TRAINING_VIT_INPUT_SIZE']
    return size, size // config['TRAINING_VIT_PATCH_SIZE'], config['GRADCAM_THRESHOLD'] if threshold is None else threshold


def window_block_labels(cells: int, window: int, device=None) -> torch.Tensor:
    """int64 [G^3]: the window^3-patch block of every patch token t = c2 G^2 + c0 G + c1, (c2 // w) Gb^2 + (c0 // w) Gb + c1 // w with
    Gb = ceil(G / w) - the blocks tile the patch grid from its origin, the last block of an axis smaller when w does not divide G
    (occlusion_sensitivity's blocks, shapley_values' default players)."""
    G, w = cells, window
    Gb = -(-G // w)
    t = torch.arange(G ** 3, device=device, dtype=torch.int64)
    c2, c0, c1 = t // (G * G), (t // G) % G, t % G
    return (c2 // w) * Gb * Gb + (c0 // w) * Gb + c1 // w


def atlas_to_patch_features(atlas: torch.Tensor, patch: int, background: int = 0):
    """An integer atlas [S, S, S] in the layout of a volume x[b] ([H, W, D]) -> (features int32 [N], labels int64 [F]): the players of
    shapley_values(features=...) on the patch grid, in token order.  Every patch takes the label most of its voxels carry (ties to the
    lower label); a patch whose label is `background` gets -1 (no player); the other labels are renumbered densely in ascending order,
    labels[f] being the atlas label of player f.  A one-off table builder in torch, on the atlas' device."""
    if atlas.dim() != 3 or atlas.is_floating_point() or atlas.dtype == torch.bool:
        raise ValueError(f"atlas_to_patch_features: atlas must be an integer tensor [S, S, S], got {atlas.dtype} {tuple(atlas.shape)}")
    p = int(patch)
    if p < 1 or any(s % p for s in atlas.shape):
        raise ValueError(f"atlas_to_patch_features: atlas {tuple(atlas.shape)} is not a whole number of {p}^3 patches")
    G0, G1, G2 = (s // p for s in atlas.shape)
    known, index = torch.unique(atlas.long(), return_inverse=True)                       # ascending
    rows = index.view(G0, p, G1, p, G2, p).permute(4, 0, 2, 1, 3, 5).reshape(G0 * G1 * G2, p ** 3)      # token order: axis 2 slowest, then 0, then 1
    counts = torch.zeros((rows.shape[0], known.numel()), dtype=torch.int64, device=atlas.device)
    counts.scatter_add_(1, rows, torch.ones_like(rows))
    majority = known[counts.argmax(dim=1)]                                               # the first maximum: the lower label
    players = torch.unique(majority[majority != background])
    features = torch.searchsorted(players, majority)                                     # (a background label lands anywhere: replaced below)
    features = torch.where(majority == background, torch.full_like(features, -1), features)
    return features.to(torch.int32).contiguous(), players


SHAPLEY_MAX_LABEL_CELLS = 2 ** 26


PATH_METHODS = ("gausslegendre", "riemann_middle", "riemann_trapezoid")


def path_quadrature(method: str, steps: int, device=None):
    """(alphas fp32 [steps], weights fp32 [steps]) of a quadrature rule on [0, 1] for integrated gradients, computed in float64 on the host:
      riemann_middle     alpha_k = (k + 1/2) / m, w_k = 1 / m;
      riemann_trapezoid  m >= 2: alpha_k = k / (m - 1), w_k = 1 / (m - 1) with the two end weights halved;
      gausslegendre      numpy.polynomial.legendre.leggauss(m) mapped from [-1, 1] to [0, 1] (captum's default rule; exact to degree 2 m - 1).
    The weights sum to 1 within fp32 rounding.  Bad arguments raise ValueError."""
    import numpy as np
    if method not in PATH_METHODS:
        raise ValueError(f"path_quadrature: method must be one of {', '.join(repr(m) for m in PATH_METHODS)}, got {method!r}")
    if isinstance(steps, bool) or int(steps) != steps or steps < 1:
        raise ValueError(f"path_quadrature: steps must be a positive integer, got {steps!r}")
    m = int(steps)
    if method == "riemann_middle":
        alphas, weights = (np.arange(m, dtype=np.float64) + 0.5) / m, np.full(m, 1.0 / m, dtype=np.float64)
    elif method == "riemann_trapezoid":
        if m < 2:
            raise ValueError(f"path_quadrature: the trapezoid rule needs at least 2 steps, got {steps!r}")
        alphas, weights = np.arange(m, dtype=np.float64) / (m - 1), np.full(m, 1.0 / (m - 1), dtype=np.float64)
        weights[0] *= 0.5
        weights[-1] *= 0.5
    else:
        nodes, w = np.polynomial.legendre.leggauss(m)
        alphas, weights = 0.5 * (nodes + 1.0), 0.5 * w
    return (torch.from_numpy(alphas).to(dtype=torch.float32, device=device), torch.from_numpy(weights).to(dtype=torch.float32, device=device))


class NeuroEncoder(nn.Module):
    """3D or 4D encoder for MRI / fMRI volumes (NeuroEncoder.py:15-68).  Attribute names and the ORDER in which sub-modules are created
    are the contract (state_dict keys; the RNG stream of a seeded construction) - tests/test_boundary_cpu.py pins both."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.device = config['DEVICE']
        self.volume_encoder = ViT3DEncoder(config)
        four_d = config['TRAINING_DIM'] == 4
        if four_d:
            self._adopt_trained_encoder(os.path.join(config['GLOBAL_BASE_PATH'], config['BEST_MODEL_PATH']))
            self.temporal_transformer = TemporalTransformer(config)
            self.projection_head = ProjectionHead(config)
            # the two modules above hold the parameters (reference classes, keys and initialisation); the computation
            # transformer -> mean over time -> projection is one native launch per direction (temporal.py, csrc/temporal.hip)
            from .temporal import TemporalHead
            self._temporal_head = TemporalHead(self.temporal_transformer, self.projection_head)
        self.to(self.device)
        self.register_hooks()

    def _adopt_trained_encoder(self, checkpoint_path: str) -> None:
        """4D model (NeuroEncoder.py:23-36): the spatial encoder is the ViT3D of a trained 3D checkpoint - loaded strictly, frozen and
        kept in eval mode; only the temporal head trains.  The file is read with weights_only=True (a plain state_dict, Trainer.py:54-55)."""
        saved = torch.load(checkpoint_path, map_location='cpu', weights_only=True)
        self.volume_encoder.load_state_dict(_encoder_weights_of(saved), strict=True)
        self.volume_encoder.requires_grad_(False)
        self.volume_encoder.eval()

    def forward(self, fmri):
        if self.config['TRAINING_DIM'] == 3:
            return self.volume_encoder(fmri)                          # NeuroEncoder.py:50-51
        if self.config['TRAINING_DIM'] != 4:
            raise ValueError(f"TRAINING_DIM must be 3 or 4, got {self.config['TRAINING_DIM']!r}")
        # 4D (NeuroEncoder.py:53-66): every timepoint is an independent volume for the frozen ViT3D, so the time axis is
        # folded into the batch; the B*T logit pairs then form a length-T sequence for the temporal transformer.
        per_volume = self._volume_logits(fmri.to(self.device))
        head = self._temporal_head
        if head.supported(per_volume):                                # NeuroEncoder.py:60-66 in one launch
            return head(per_volume)
        # geometries outside the kernel's (more than 64 timepoints, an edited encoder layer): the stock modules, on the device
        pooled = self.temporal_transformer(per_volume).mean(dim=1)
        return self.projection_head(pooled)

    def _volume_logits(self, series):
        """[B, H, W, D, T] on the device -> the frozen encoder's logits of every timepoint [B, T, 2]"""
        n_samples, n_time = series.shape[0], series.shape[-1]
        vit = self.volume_encoder.vit3d
        # the fused form records no graph: only when neither the encoder's parameters nor the series (dL/d fMRI) want a gradient
        frozen = not (torch.is_grad_enabled() and (series.requires_grad or any(p.requires_grad for p in vit.parameters())))
        patch_dim = self.config['TRAINING_VIT_PATCH_SIZE'] ** 3
        if frozen and n_time % 4 == 0 and n_time <= 64 and patch_dim % 4 == 0 and series.dtype == torch.float32 and series.is_contiguous():
            # fused 4D gather (csrc/norm.hip::patch_ln_fwd_t_kernel: float4 groups, so not for the 9^3 patches of the reference's 90^3
            # geometry): the B*T volumes are read in place, no regroup copy
            return vit(series, time_points=n_time).unflatten(0, (n_samples, n_time))
        as_volumes = series.movedim(-1, 1).flatten(0, 1)              # [B, H, W, D, T] -> [B*T, H, W, D]  (strided copy)
        return self.volume_encoder(as_volumes).unflatten(0, (n_samples, n_time))

    @property
    def is_regression(self) -> bool:
        return bool(getattr(self.volume_encoder, "regression", False))

    def predict(self, x):
        """Regression model (TRAINING_OBJECTIVE "regression"): predictions [B, K] on the RAW scale - the head's outputs times
        REGRESSION_TARGET_STD plus REGRESSION_TARGET_MEAN - from a no-grad forward in the module's current mode."""
        if not self.is_regression:
            raise RuntimeError("NeuroEncoder.predict: the model is a classifier - build it with TRAINING_OBJECTIVE 'regression'")
        enc = self.volume_encoder
        with torch.no_grad():
            return self(x).float() * enc.target_std + enc.target_mean

    def extract_features(self, x, pool=None, normalize=False, out=None, row0=0):
        """x [B, H, W, D] -> fp32 [B, dim]: one frozen embedding per volume (ViT.forward_features behind this encoder's permute: the eval-mode
        forward of the encoder's eval_precision, no graph, no .grad touched).  pool None = the model's own pooling, "cls", "mean" or
        "patch_mean"; normalize = F.normalize's rule; out / row0 fill rows of a preallocated bank (features.FeatureBank).  3D model only: the
        4D model's per-volume "encoding" is its two logits, not an embedding."""
        if self.config['TRAINING_DIM'] != 3:
            raise NotImplementedError("NeuroEncoder.extract_features: 3D model only - the 4D model's per-volume encoding is two logits, not an "
                                      "embedding; extract features with its (3D) volume encoder's checkpoint")
        if x.dim() != 4:
            raise ValueError(f"NeuroEncoder.extract_features: expected volumes [B, H, W, D], got {tuple(x.shape)}")
        volume = x.to(self.device)
        return self.volume_encoder.vit3d.forward_features(volume.permute(0, 3, 1, 2).unsqueeze(1), pool=pool, normalize=normalize, out=out, row0=row0)

    def precision(self, mode: str):
        """Context manager: eval-mode no-grad forwards of the ViT3D encoder inside it run in `mode` ("bf16" / "fp16": the 16-bit
        operand path in the encoder's operand format, or "fp32")."""
        return self.volume_encoder.vit3d.precision(mode)

    def set_operands(self, fmt: str):
        """16-bit MFMA operand format of the ViT3D encoder: "bf16" (default) or "fp16" (the reference's autocast arithmetic)."""
        self.volume_encoder.vit3d.set_operands(fmt)
        return self

    def forward_raw(self, raw, crop=None):
        """3D model fed RAW scanner volumes [B, X, Y, Z] float32 on the device: the dataset's crop (DatasetADNI.py:212) is a strided
        view and its z-score (:213) is folded into the patch LayerNorm - one statistics pass, no normalised copy."""
        if self.config['TRAINING_DIM'] != 3:
            raise NotImplementedError("forward_raw: 3D model only (4D samples are normalised over all timepoints: DatasetADNI_4D.py:86-87)")
        return self.volume_encoder.forward_raw(raw, crop)

    # ---- Grad-CAM contract (NeuroEncoder.py:70-82): activation / gradient of the last block's attention-LN output.
    # The reference copies both to the CPU on EVERY forward / backward (a blocking D2H sync per step); here they stay
    # in the engine workspace and are materialised on attribute access only.
    def register_hooks(self):
        self._hook_override = {}

    @property
    def activations(self):
        if 'activations' in self._hook_override:
            return self._hook_override['activations']
        vit = self.volume_encoder.vit3d
        if vit._rt.last is None:
            return {}
        return vit.last_attn_norm_output().detach().cpu()

    @activations.setter
    def activations(self, value):
        self._hook_override['activations'] = value

    @property
    def gradients(self):
        if 'gradients' in self._hook_override:
            return self._hook_override['gradients']
        vit = self.volume_encoder.vit3d
        # the buffer holds the gradient only once a backward pass of the most recent training-mode forward has run
        last = vit._rt.last
        if last is None or not last.layout or not last.grad_ready:
            return {}
        return vit.last_attn_norm_grad().detach().cpu()

    @gradients.setter
    def gradients(self, value):
        self._hook_override['gradients'] = value

    def get_attention_map(self, x):
        """Grad-CAM of the predicted class on the patch grid, thresholded and upsampled to the volume
        (same contract as NeuroEncoder.py:84-133: returns (cam[S,S,S] on the CPU, class_idx)).

        The [B,n,d] activation and gradient never leave the device: `nv_gradcam_reduce` (csrc/attribution.hip) turns them
        into the normalised G^3 map in one launch, and only those G^3 floats cross PCIe for the percentile / upsampling."""
        from . import ops
        logits = self.forward(x)
        predicted = logits.argmax(dim=1)
        logits.backward(gradient=F.one_hot(predicted, logits.shape[1]).to(logits.dtype), retain_graph=True)

        vit = self.volume_encoder.vit3d
        if 'activations' in self._hook_override or 'gradients' in self._hook_override:      # user-assigned hook tensors win
            act, grad = self.activations.float(), self.gradients.float()
            token_map = torch.relu(grad.mean(dim=2) * act.sum(dim=2))[:, 1:]
            token_map = (token_map - token_map.min()) / (token_map.max() - token_map.min() + 1e-8)
        else:
            token_map, _ = ops.gradcam_reduce(vit.last_attn_norm_output_raw(), vit.last_attn_norm_grad_raw())
            token_map = token_map.cpu()
        return self._token_map_to_volume(token_map), predicted

    def _token_map_to_volume(self, token_map, normalize=False):
        """[1, G^3] CPU map of the patch tokens -> [S, S, S]: min-max normalised over the map (normalize; else it arrives normalised), the
        top GRADCAM_THRESHOLD % of the cells (linear-interpolated percentile, as numpy.percentile), the rest zeroed, trilinear upsampling
        to the volume (NeuroEncoder.py:120-131)."""
        size, cells, keep_percent = _grid_geometry(self.config)
        if normalize:
            token_map = (token_map - token_map.min()) / (token_map.max() - token_map.min() + 1e-8)
        grid = token_map.reshape(1, cells, cells, cells)               # one sample, as in the reference
        cut = torch.quantile(grid.double().flatten(), 1.0 - keep_percent / 100.0).to(grid.dtype)
        sparse = torch.where(grid >= cut, grid, torch.zeros_like(grid))
        volume = F.interpolate(sparse[None], size=(size,) * 3, mode='trilinear', align_corners=False)
        return volume[0, 0]

    def get_attention_rollout(self, x):
        """Attention rollout of the ViT3D encoder on the patch grid, in the form of get_attention_map: (map[S,S,S] on the CPU, class_idx),
        so visualize_slice and Grad-CAM plotting code take it unchanged.  The cls row of the head-averaged, identity-augmented attention
        multiplied over the layers (ViT.attention_rollout: one forward in the module's current mode and precision, no backward pass),
        min-max normalised over the map, thresholded and upsampled as get_attention_map does."""
        if self.config['TRAINING_DIM'] != 3:
            raise NotImplementedError("get_attention_rollout: 3D model only (as get_attention_map, one volume [1, H, W, D])")
        vit = self.volume_encoder.vit3d
        volume = x.to(self.device)
        with torch.no_grad():
            logits, rollout = vit.attention_rollout(volume.permute(0, 3, 1, 2).unsqueeze(1))     # ViT3DEncoder.forward's view
        return self._token_map_to_volume(rollout.cpu(), normalize=True), logits.argmax(dim=1)

    def get_attention_relevance(self, x, target=None):
        """Class-specific attention relevance of the ViT3D encoder on the patch grid (gradient-weighted attention relevance, Chefer et al.:
        mean_h relu(grad A * A) accumulated over the layers), in the form of get_attention_map: (map[S,S,S] on the CPU, class_idx).  Unlike
        the rollout it depends on the class: `target` None explains the predicted class (as get_attention_map), an int or a LongTensor
        that class; class_idx is the explained class.  One forward and one data-only backward (ViT.attention_relevance: no p.grad is
        touched, no autograd graph needed), min-max normalised over the map, thresholded and upsampled as get_attention_map does."""
        if self.config['TRAINING_DIM'] != 3:
            raise NotImplementedError("get_attention_relevance: 3D model only (as get_attention_map, one volume [1, H, W, D])")
        vit = self.volume_encoder.vit3d
        volume = x.to(self.device)
        logits, relevance = vit.attention_relevance(volume.permute(0, 3, 1, 2).unsqueeze(1), target=target)   # ViT3DEncoder.forward's view
        return self._token_map_to_volume(relevance.cpu(), normalize=True), target_classes(target, logits)

    # ---- batched attribution, on the device (csrc/attribution.hip): the three maps above for a whole batch, every volume on its own
    def token_maps_to_volumes(self, token_maps, normalize=True, threshold=None):
        """[B, G^3] maps of the patch tokens (device, token order) -> fp32 [B, S, S, S] on the device: what _token_map_to_volume does to
        one CPU map, for every volume of the batch independently and without leaving the device (nv_token_map_to_volume) - min-max
        normalisation over the volume's own cells (normalize), the top `threshold` % of its cells kept (None: GRADCAM_THRESHOLD;
        torch.quantile's linear rule), trilinear upsampling to the volume.  The building block for any map on the patch grid."""
        from . import ops
        size, cells, keep_percent = _grid_geometry(self.config, threshold)
        maps = token_maps.to(device=self.device, dtype=torch.float32).contiguous()
        return ops.token_maps_to_volumes(maps, cells, size, normalize=normalize, keep_percent=keep_percent)

    def attribution_volumes(self, x, method="gradcam", target=None, threshold=None, return_token_maps=False):
        """Attribution volumes of a batch x [B, H, W, D]: (volumes fp32 [B, S, S, S] on the device, class_idx [B] on the device[, the
        normalised token maps [B, G^3] on the device]).  method "gradcam" / "rollout" / "relevance" runs the GPU steps of
        get_attention_map / get_attention_rollout / get_attention_relevance on the whole batch, in the module's current mode; "occlusion" is
        relu(occlusion_sensitivity(x, target)) - G^3 + 1 forwards per volume, no gradient and no assumption about attention;
        "integrated_gradients" is relu of the token_maps of integrated_gradients(x, target) with its defaults (zero baseline, 50
        Gauss-Legendre points, the class logit: 50 forward + data-only backward passes per volume, no p.grad touched); "shapley" is relu of
        the token_maps of shapley_values(x, target) with its defaults (2^3-patch blocks, 16 antithetic permutations: 2 + 16 (F - 1) forwards
        per volume):
          gradcam    one forward, logits.backward(one-hot) with one row per volume (the logits are per volume: volumes do not couple),
                     the per-volume reduction nv_gradcam_reduce_per_volume.  As get_attention_map it runs the model's backward pass:
                     a trainable model accumulates p.grad; a frozen one runs the data-only backward and touches none;
          rollout    ViT.attention_rollout; `target` is ignored for the map, class_idx is the predicted class;
          relevance  ViT.attention_relevance (one forward, one data-only backward; no p.grad is touched).
        target: None = the predicted class of each volume, an int, or a LongTensor [B]; class_idx is the explained class.
        Every volume is normalised, thresholded (threshold: percent of cells kept, None = GRADCAM_THRESHOLD) and upsampled on its own
        (token_maps_to_volumes).  No tensor crosses PCIe and nothing synchronises with the host inside the call.
        User-assigned `model.activations` / `model.gradients` overrides are NOT consulted (get_attention_map honours them)."""
        from . import ops
        target = self._resolve_target(target)             # (a regression model: output 0; the score-based methods resolve their score to "logit")
        if self.config['TRAINING_DIM'] != 3:
            raise NotImplementedError("attribution_volumes: 3D model only (as get_attention_map; the 4D model has no patch-grid attribution)")
        if method not in ("gradcam", "rollout", "relevance", "occlusion", "integrated_gradients", "shapley"):
            raise ValueError("attribution_volumes: method must be 'gradcam', 'rollout', 'relevance', 'occlusion', 'integrated_gradients' or 'shapley', "
                             f"got {method!r}")
        vit = self.volume_encoder.vit3d
        normalize = True
        if method == "occlusion":
            # the signed occlusion map (one patch per job, zero baseline, probability score); the volume shows what SUPPORTS the class
            signed, class_idx = self.occlusion_sensitivity(x, target=target)
            token_maps = torch.relu(signed)
        elif method == "integrated_gradients":
            # the signed patch sums of integrated gradients (zero baseline, 50 Gauss-Legendre points, the class logit)
            result = self.integrated_gradients(x, target=target)
            token_maps, class_idx = torch.relu(result["token_maps"]), result["class_idx"]
        elif method == "shapley":
            # the signed Shapley values of the 2^3-patch blocks (16 antithetic permutations, zero baseline, probability score), spread over the patches
            result = self.shapley_values(x, target=target)
            token_maps, class_idx = torch.relu(result["token_maps"]), result["class_idx"]
        elif method == "gradcam":
            volume = x.to(self.device)
            with torch.enable_grad():
                if not (volume.requires_grad or any(p.requires_grad for p in vit.parameters())):
                    volume = volume.detach().requires_grad_(True)       # a frozen model: the data-only backward delivers the hook gradient
                logits = self.forward(volume)
                class_idx = target_classes(target, logits.detach())
                logits.backward(gradient=F.one_hot(class_idx, logits.shape[1]).to(logits.dtype))
            token_maps, _ = ops.gradcam_reduce_per_volume(vit.last_attn_norm_output_raw(), vit.last_attn_norm_grad_raw())
            normalize = False                                           # the reduction has normalised every volume
        else:
            video = x.to(self.device).permute(0, 3, 1, 2).unsqueeze(1)     # ViT3DEncoder.forward's view
            if method == "rollout":
                with torch.no_grad():
                    logits, token_maps = vit.attention_rollout(video)
                class_idx = logits.argmax(dim=1)
            else:
                logits, token_maps = vit.attention_relevance(video, target=target)
                class_idx = target_classes(target, logits)

        size, cells, keep_percent = _grid_geometry(self.config, threshold)
        volumes, (normalised, _, _) = ops.token_maps_to_volumes(token_maps.contiguous(), cells, size, normalize=normalize, keep_percent=keep_percent,
                                                                return_maps=True)
        return (volumes, class_idx, normalised) if return_token_maps else (volumes, class_idx)

    # ---- perturbation attribution, on the device (csrc/perturb.hip): how faithful a map is (deletion / insertion curves) and the
    # gradient-free baseline among the maps (patch occlusion sensitivity)
    def _resolve_score(self, what, score, default="prob"):
        """score None = `default` on a classifier, "logit" on a regression model - where "prob" means nothing (the softmax of one output is
        1, of several a competition between unrelated targets) and is refused"""
        if score is None:
            return "logit" if self.is_regression else default
        if self.is_regression and score == "prob":
            raise ValueError(f"{what}: score 'prob' is meaningless on a regression model (its outputs are predictions, not class logits) - use "
                             "score='logit' (or None), the output itself")
        return score

    def _resolve_target(self, target):
        """target None on a regression model = output 0 (there is no predicted class to fall back to)"""
        return 0 if target is None and self.is_regression else target

    def _perturbation_inputs(self, what, x, baseline, score, chunk):
        """argument checks shared by perturbation_curves / occlusion_sensitivity (all before any device work) -> (S, G, chunk)"""
        from . import ops
        if self.config['TRAINING_DIM'] != 3:
            raise NotImplementedError(f"{what}: 3D model only (as get_attention_map; the 4D model has no patch-grid attribution)")
        if score not in ("prob", "logit"):
            raise ValueError(f"{what}: score must be 'prob' or 'logit', got {score!r}")
        S = self.config['TRAINING_VIT_INPUT_SIZE']
        if x.dim() != 4 or tuple(x.shape[1:]) != (S, S, S) or x.shape[0] < 1:
            raise ValueError(f"{what}: x must be [B, {S}, {S}, {S}], got {tuple(x.shape)}")
        ops.check_baseline(what, baseline, x.shape)
        if chunk is None:
            chunk = max(1, min(64, 2 ** 30 // (4 * S ** 3)))
        elif int(chunk) != chunk or chunk < 1:
            raise ValueError(f"{what}: chunk must be a positive integer, got {chunk!r}")
        return S, S // self.config['TRAINING_VIT_PATCH_SIZE'], int(chunk)

    def _perturbed_logits(self, volume, labels, jobs, baseline, chunk):
        """logits [J, C] of the masked copies of `volume`: consecutive slices of `chunk` jobs, each masked into one reused buffer and
        forwarded under no_grad in the module's current mode and precision.  jobs [J, 3] = (b, lo, hi) with labels [B, N]
        (ops.mask_patches), or jobs [J, 4] = (b, row, lo, hi) with labels [Rows, N] (ops.mask_patches_rows)"""
        from . import ops
        patch = self.config['TRAINING_VIT_PATCH_SIZE']
        J = jobs.shape[0]
        mask = ops.mask_patches_rows if jobs.shape[1] == 4 else ops.mask_patches
        chunk = min(chunk, J)
        if torch.is_tensor(baseline):
            baseline = baseline.to(device=volume.device, dtype=torch.float32).contiguous()
        masked = torch.empty((chunk,) + tuple(volume.shape[1:]), dtype=torch.float32, device=volume.device)
        logits = None
        with torch.no_grad():
            for first in range(0, J, chunk):
                count = min(chunk, J - first)
                mask(volume, labels, jobs[first:first + count], patch, baseline=baseline, out=masked[:count])
                part = self.forward(masked[:count])
                if logits is None:
                    logits = torch.empty((J, part.shape[1]), dtype=torch.float32, device=volume.device)
                logits[first:first + count].copy_(part)
        return logits

    def perturbation_curves(self, x, token_maps, target=None, steps=20, mode="both", baseline=0.0, score=None, chunk=None):
        """Deletion / insertion curves of token maps [B, G^3] (token order, e.g. the third result of attribution_volumes(...,
        return_token_maps=True)) for a batch x [B, H, W, D]: the class score while the patches are replaced by the baseline (deletion) or
        restored into the baseline (insertion) in the order the map ranks them - a faithful map has a small deletion area and a large
        insertion area.  target: None = the predicted class of the unperturbed volume, an int, or a LongTensor [B].
          ranks      ops.token_ranks(token_maps): descending, ties to the lower token index (thresholded maps are mostly ties);
          steps      K = steps + 1 points; point k has the m_k = (2 k N + steps) // (2 steps) top-ranked of the N patches removed (deletion)
                     or present (insertion): m_0 = 0, m_steps = N;
          jobs       volume-major; within a volume deletion k = 0 .. steps = (b, 0, m_k), then insertion k = 0 .. steps = (b, m_k, N), the
                     labels being the ranks (ops.mask_patches); consecutive slices of `chunk` jobs (None: max(1, min(64, 2^30 // (4 S^3))))
                     are masked into one reused buffer and forwarded under no_grad in the module's current mode and precision;
          baseline   a float, or a tensor of x's shape or [1, S, S, S] (a blurred copy, a mean volume);
          score      "prob" (softmax probability of the class) or "logit"; None = "prob" on a classifier, "logit" on a regression model
                     (TRAINING_OBJECTIVE "regression": "prob" is refused there, and target None means output 0).
        Returns a dict of device tensors: deletion / insertion [B, K], deletion_auc / insertion_auc [B] (trapezoid rule over
        fractions = k / steps [K]), class_idx [B], ranks [B, N]; mode "deletion" / "insertion" computes and returns only that pair.
        Nothing crosses PCIe and nothing synchronises with the host inside the call."""
        from . import ops
        score, target = self._resolve_score("perturbation_curves", score), self._resolve_target(target)
        S, G, chunk = self._perturbation_inputs("perturbation_curves", x, baseline, score, chunk)
        if mode not in ("both", "deletion", "insertion"):
            raise ValueError(f"perturbation_curves: mode must be 'both', 'deletion' or 'insertion', got {mode!r}")
        if int(steps) != steps or steps < 1:
            raise ValueError(f"perturbation_curves: steps must be a positive integer, got {steps!r}")
        steps, N, B = int(steps), G ** 3, x.shape[0]
        if tuple(token_maps.shape) != (B, N):
            raise ValueError(f"perturbation_curves: token_maps must be [{B}, {N}] (one value per patch token), got {tuple(token_maps.shape)}")
        K = steps + 1
        volume = x.to(device=self.device, dtype=torch.float32).contiguous()
        device = volume.device

        def build():
            m = perturbation_step_bounds(N, steps, device)
            zero, full = torch.zeros_like(m), torch.full_like(m, N)
            bounds = {"both": torch.cat([torch.stack([zero, m], 1), torch.stack([m, full], 1)]), "deletion": torch.stack([zero, m], 1),
                      "insertion": torch.stack([m, full], 1)}[mode]                                  # [K or 2 K, 2]: (lo, hi)
            source = torch.arange(B, device=device, dtype=torch.int64).repeat_interleave(bounds.shape[0])
            return torch.cat([source[:, None], bounds.repeat(B, 1)], 1).to(torch.int32).contiguous(), (torch.arange(K, device=device, dtype=torch.float64) / steps).float()
        jobs, fractions = cached_table(self, "_perturbation_tables", ("curves", str(device), B, N, steps, mode), build)

        with torch.no_grad():
            class_idx = target_classes(target, self.forward(volume))
        ranks = ops.token_ranks(token_maps.to(device=device, dtype=torch.float32).contiguous())
        logits = self._perturbed_logits(volume, ranks, jobs, baseline, chunk)
        scores = ops.class_scores(logits, jobs, class_idx, kind=score).view(B, -1)
        out = {"fractions": fractions, "class_idx": class_idx, "ranks": ranks}
        for name, first in (("deletion", 0), ("insertion", K if mode == "both" else 0)):
            if mode in ("both", name):
                out[name] = scores[:, first:first + K]
                out[name + "_auc"] = ops.curve_auc(out[name])
        return out

    def occlusion_sensitivity(self, x, target=None, window=1, baseline=0.0, score=None, chunk=None):
        """Patch occlusion sensitivity of a batch x [B, H, W, D]: (maps fp32 [B, G^3] in token order, class_idx [B]), both on the device.
        maps[b, t] = score of x[b] - score of x[b] with the window^3-patch block that holds patch t replaced by the baseline: signed
        (positive = the block supports the class), no gradient and no assumption about attention.  The blocks tile the patch grid from
        its origin (the last block of an axis is smaller when window does not divide G): cell (c2, c0, c1) of token t = c2 G^2 + c0 G + c1
        lies in block (c2 // w) Gb^2 + (c0 // w) Gb + c1 // w, Gb = ceil(G / w); one job (b, j, j + 1) per volume and block, volume-major,
        masked and forwarded in slices of `chunk` jobs as perturbation_curves does.  One more forward of x gives the unperturbed score and,
        with target None, the predicted class.  target / baseline / score / chunk: as perturbation_curves.  Costs Gb^3 + 1 forwards per
        volume; nothing crosses PCIe and nothing synchronises with the host inside the call."""
        from . import ops
        score, target = self._resolve_score("occlusion_sensitivity", score), self._resolve_target(target)
        S, G, chunk = self._perturbation_inputs("occlusion_sensitivity", x, baseline, score, chunk)
        if int(window) != window or window < 1:
            raise ValueError(f"occlusion_sensitivity: window must be a positive integer, got {window!r}")
        w, N, B = int(window), G ** 3, x.shape[0]
        Gb = -(-G // w)
        NB = Gb ** 3
        volume = x.to(device=self.device, dtype=torch.float32).contiguous()
        device = volume.device

        def build():
            block = window_block_labels(G, w, device)
            b = torch.arange(B, device=device, dtype=torch.int64)
            j = torch.arange(NB, device=device, dtype=torch.int64).repeat(B)
            jobs = torch.stack([b.repeat_interleave(NB), j, j + 1], 1).to(torch.int32).contiguous()
            plain = torch.stack([b, torch.zeros_like(b), torch.zeros_like(b)], 1).to(torch.int32).contiguous()      # rows (b, 0, 0): x itself
            return block.to(torch.int32).repeat(B, 1).contiguous(), jobs, plain
        labels, jobs, plain = cached_table(self, "_perturbation_tables", ("occlusion", str(device), B, G, w), build)

        with torch.no_grad():
            unperturbed = self.forward(volume).float().contiguous()
        class_idx = target_classes(target, unperturbed)
        reference = ops.class_scores(unperturbed, plain, class_idx, kind=score)
        logits = self._perturbed_logits(volume, labels, jobs, baseline, chunk)
        scores = ops.class_scores(logits, jobs, class_idx, kind=score).view(B, NB)
        return ops.occlusion_gather(reference, scores, labels), class_idx

    # ---- Shapley value sampling, on the device (csrc/shapley.hip): the one attribution that is efficient and order-free, over patches,
    # blocks of patches or atlas regions
    def shapley_values(self, x, target=None, permutations=16, window=2, features=None, antithetic=True, baseline=0.0, score=None, seed=0,
                       permutation_offset=0, ranks=None, chunk=None, return_scores=False):
        """Shapley values of players on the patch grid for a batch x [B, H, W, D], by permutation sampling (Castro et al.; captum's
        ShapleyValueSampling): the mean over random orders of the change in the class score when a player joins the players before it.
        The values of a volume sum to score(x) - score(everything at the baseline) (efficiency), whatever the order of the players.
          players    features None: the window^3-patch blocks of occlusion_sensitivity (window_block_labels; window 1 = one player per
                     patch).  Otherwise an int tensor [N] or [B, N] of player ids in token order, -1 = no player (such a patch stays as in x
                     in every copy), F = max + 1 (with ranks: its last dimension): an atlas on the patch grid (atlas_to_patch_features).
                     F is read on the host: a CPU tensor costs nothing, a device tensor one read-back.  2 <= F <= 4096;
          draw       nv_shapley_ranks (the rule is in the header): antithetic needs an even `permutations` P and draws U = P / 2 units of a
                     permutation and its reverse (R = 2); otherwise U = P, R = 1.  The units drawn are permutation_offset ..
                     permutation_offset + U - 1, so two calls can draw disjoint permutations.  ranks int [P, F] or [P, B, F] (rank of every
                     player, a permutation per row) replaces the draw: R = 1, antithetic is ignored, and every row is checked to be a
                     permutation in torch - the one host synchronisation of that path;
          jobs       (b, row, lo, hi) for ops.mask_patches_rows over the labels ops.shapley_labels(ranks, features) [P B, N] (row q B + b:
                     permutation q of volume b; label = the rank of the patch's player, F for no player), in one global order: first the
                     ends, volume-major, (b, b, 0, F) - every player at the baseline - then (b, b, F, F) - x itself; then for permutation
                     q = 0 .. P - 1, volume b, k = 1 .. F - 1: (b, q B + b, k, F) - the k first-ranked players present.  Consecutive slices
                     of `chunk` jobs of this list are masked and forwarded as perturbation_curves does;
          values     ops.shapley_accumulate: the marginal of player f of rank rho in a permutation is s_{rho+1} - s_rho; a unit's value is
                     the mean of its R marginals; values = the mean over the units, stderr its standard error (NaN for U = 1).
        target / baseline / score / chunk: as perturbation_curves.  Costs B (2 + P (F - 1)) forwards.  More than 2^26 label cells
        (P B N) are refused: split the permutations over calls with permutation_offset and average.
        Returns a dict of device tensors: values / stderr [B, F], token_maps [B, N] (a player's value spread evenly over its patches:
        what token_maps_to_volumes and perturbation_curves take), class_idx [B], full_score / empty_score [B], delta [B] (sum of the values
        - (full - empty), the efficiency residual: rounding only), feature_labels int32 [B, N], ranks int32 [P, B, F]; with return_scores
        also interior [P, B, F - 1] and ends [B, 2] (empty, full).  Without ranks= nothing synchronises with the host inside the call."""
        from . import ops
        what = "shapley_values"
        score, target = self._resolve_score(what, score), self._resolve_target(target)
        S, G, chunk = self._perturbation_inputs(what, x, baseline, score, chunk)
        N, B = G ** 3, x.shape[0]
        if ranks is not None:
            if not torch.is_tensor(ranks) or ranks.is_floating_point() or ranks.dim() not in (2, 3) or (ranks.dim() == 3 and ranks.shape[1] != B):
                raise ValueError(f"{what}: ranks must be an int tensor [P, F] or [P, {B}, F], got {tuple(ranks.shape) if torch.is_tensor(ranks) else ranks!r}")
            P, F_given = ranks.shape[0], ranks.shape[-1]
            U, R = P, 1
        else:
            if isinstance(permutations, bool) or int(permutations) != permutations or permutations < 1:
                raise ValueError(f"{what}: permutations must be a positive integer, got {permutations!r}")
            P, F_given = int(permutations), None
            if antithetic and P % 2:
                raise ValueError(f"{what}: antithetic sampling draws pairs of permutations and needs an even number, got permutations = {P}")
            U, R = (P // 2, 2) if antithetic else (P, 1)
            if int(permutation_offset) != permutation_offset or permutation_offset < 0 or permutation_offset + U > 2 ** 32:
                raise ValueError(f"{what}: permutation_offset must be an integer in [0, 2^32 - {U}], got {permutation_offset!r}")
        if features is None:
            if int(window) != window or window < 1:
                raise ValueError(f"{what}: window must be a positive integer, got {window!r}")
            w = int(window)
            F = (-(-G // w)) ** 3
            feature_key = ("blocks", w)
        else:
            if not torch.is_tensor(features) or features.is_floating_point() or tuple(features.shape) not in ((N,), (B, N)):
                raise ValueError(f"{what}: features must be an int tensor [{N}] or [{B}, {N}] of player ids, got "
                                 f"{tuple(features.shape) if torch.is_tensor(features) else features!r}")
            top = int(features.max())
            F = top + 1 if F_given is None else F_given
            if top >= F:
                raise ValueError(f"{what}: features name player {top}, ranks has {F} players")
            feature_key = None
        if F_given is not None and F_given != F:
            raise ValueError(f"{what}: ranks has {F_given} players, the window {window} gives {F}")
        if F < 2 or F > ops.SHAPLEY_MAX_PLAYERS:
            raise ValueError(f"{what}: {F} players, needs 2 <= F <= {ops.SHAPLEY_MAX_PLAYERS}")
        if P * B * N > SHAPLEY_MAX_LABEL_CELLS:
            raise ValueError(f"{what}: {P} permutations x {B} volumes x {N} patches = {P * B * N} label cells, more than 2^26: split the permutations "
                             "over several calls with permutation_offset and average the values")
        volume = x.to(device=self.device, dtype=torch.float32).contiguous()
        device = volume.device

        if feature_key is None:
            feature_labels = features.to(device=device, dtype=torch.int32).expand(B, N).contiguous()
        else:
            feature_labels = cached_table(self, "_perturbation_tables", ("shapley players", str(device), B, G) + feature_key,
                                          lambda: window_block_labels(G, w, device).to(torch.int32).repeat(B, 1).contiguous())

        def build():
            b = torch.arange(B, device=device, dtype=torch.int64)
            full = torch.full_like(b, F)
            ends = torch.stack([torch.stack([b, b, torch.zeros_like(b), full], 1), torch.stack([b, b, full, full], 1)], 1).view(2 * B, 4)
            q = torch.arange(P, device=device, dtype=torch.int64).view(P, 1, 1).expand(P, B, F - 1)
            bb = b.view(1, B, 1).expand(P, B, F - 1)
            k = torch.arange(1, F, device=device, dtype=torch.int64).view(1, 1, F - 1).expand(P, B, F - 1)
            inner = torch.stack([bb, q * B + bb, k, torch.full_like(k, F)], 3).view(P * B * (F - 1), 4)
            jobs = torch.cat([ends, inner]).to(torch.int32).contiguous()
            return jobs, jobs[:, [0, 2, 3]].contiguous()                       # the companion (b, lo, hi) table of nv_class_scores
        jobs, score_jobs = cached_table(self, "_perturbation_tables", ("shapley", str(device), B, F, P), build)

        if ranks is None:
            order = ops.shapley_ranks(U, R, B, F, seed=seed, first_unit=int(permutation_offset), device=device)
        else:
            order = ranks.to(device=device, dtype=torch.int32)
            order = (order if order.dim() == 3 else order[:, None, :].expand(P, B, F)).contiguous()
            if not bool((torch.sort(order, dim=2).values == torch.arange(F, device=device, dtype=torch.int32)).all()):      # (the host synchronisation)
                raise ValueError(f"{what}: every row of ranks must be a permutation of 0 .. {F - 1}")
        with torch.no_grad():
            class_idx = target_classes(target, self.forward(volume))
        labels = ops.shapley_labels(order, feature_labels)
        logits = self._perturbed_logits(volume, labels, jobs, baseline, chunk)
        scores = ops.class_scores(logits, score_jobs, class_idx, kind=score)
        ends, interior = scores[:2 * B].view(B, 2), scores[2 * B:].view(P, B, F - 1)
        values, stderr, delta, _ = ops.shapley_accumulate(interior, ends, order, R=R)
        out = {"values": values, "stderr": stderr, "token_maps": ops.shapley_token_maps(values, feature_labels), "class_idx": class_idx,
               "full_score": ends[:, 1], "empty_score": ends[:, 0], "delta": delta, "feature_labels": feature_labels, "ranks": order}
        if return_scores:
            out.update(interior=interior, ends=ends)
        return out

    # ---- path attribution, on the device (csrc/path_attr.hip): integrated gradients, the map the reference ships captum heat maps of
    def integrated_gradients(self, x, target=None, baseline=0.0, steps=50, method="gausslegendre", score="logit", chunk=None):
        """Integrated gradients of a batch x [B, H, W, D] (ViT.integrated_gradients on ViT3DEncoder.forward's view: the arguments, the
        passes and the side effects - none: no p.grad, no gradient arena, no host synchronisation - are described there; call eval()
        first).  baseline: a float, or a tensor of x's shape or [1, S, S, S].  steps / method: path_quadrature.  chunk None:
        max(1, min(64, 2^29 // (4 S^3))) points per pass.  It runs in the training arithmetic (16-bit operands): precision("fp32") does
        not apply.  Returns a dict of device tensors:
          attributions [B, S, S, S]; token_maps [B, G^3] the sum and token_abs [B, G^3] the sum of absolute values of every patch's
          attributions (nv_attr_token_sums; token order - what token_maps_to_volumes and perturbation_curves take); class_idx [B];
          score_input / score_baseline [B]; delta [B] float64 = sum of token_maps in double - (score_input - score_baseline), the
          completeness residual; alphas / weights [steps]."""
        from . import ops
        score, target = self._resolve_score("integrated_gradients", score, "logit"), self._resolve_target(target)
        S, G, _ = self._perturbation_inputs("integrated_gradients", x, baseline, score, 1 if chunk is None else chunk)
        path_quadrature(method, steps)                                 # (ValueError before any device work)
        volume = x.to(device=self.device, dtype=torch.float32).contiguous()
        if torch.is_tensor(baseline):
            baseline = baseline.to(device=volume.device, dtype=torch.float32).permute(0, 3, 1, 2).unsqueeze(1)
        vit = self.volume_encoder.vit3d
        out = vit.integrated_gradients(volume.permute(0, 3, 1, 2).unsqueeze(1), target=target, baseline=baseline, steps=steps, method=method,
                                       score=score, chunk=chunk)       # ViT3DEncoder.forward's view: the storage order stays [B, H, W, D]
        attributions = out["attributions"].squeeze(1).permute(0, 2, 3, 1)
        sums = ops.attr_token_sums(attributions, self.config['TRAINING_VIT_PATCH_SIZE'])
        token_maps, token_abs = sums[:, :, 0].contiguous(), sums[:, :, 1].contiguous()
        delta = token_maps.double().sum(1) - (out["score_input"].double() - out["score_baseline"].double())
        return dict(out, attributions=attributions, token_maps=token_maps, token_abs=token_abs, delta=delta)

    # ---- spatio-temporal attribution of the 4D model (csrc/series_attr.hip): which timepoints drove a class, and which regions at each
    SERIES_METHODS = ("gradcam", "rollout", "relevance")

    def _series_inputs(self, what, x, target, chunk):
        """argument checks and refusals shared by attribution_series / temporal_importance (all before any device work) -> (S, G, T, chunk)"""
        from .vit_3d import check_target
        if self.config['TRAINING_DIM'] != 4:
            raise NotImplementedError(f"{what}: 4D model only (a 3D model has no time axis: attribution_volumes serves it)")
        S = self.config['TRAINING_VIT_INPUT_SIZE']
        if x.dim() != 5 or tuple(x.shape[1:4]) != (S, S, S) or x.shape[0] < 1 or x.shape[4] < 1:
            raise ValueError(f"{what}: x must be [B, {S}, {S}, {S}, T], got {tuple(x.shape)}")
        if chunk is None:
            chunk = 64
        elif isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
            raise ValueError(f"{what}: chunk must be a positive integer, got {chunk!r}")
        check_target(target, x.shape[0], 2)
        T = x.shape[4]
        vit, head = self.volume_encoder.vit3d, self._temporal_head
        if not head.supports(T):
            raise NotImplementedError(f"{what}: the temporal head is outside what the native kernel computes (TemporalHead.supported: at most 64 "
                                      "timepoints, the stock encoder layer) - its input gradient comes from that kernel")
        if self.temporal_transformer.training and float(head._layer.dropout.p) > 0:
            raise NotImplementedError(f"{what}: the temporal head is in train mode with dropout > 0 - call eval() for attribution")
        if vit.training and max(vit._dropout_p) > 0:
            raise NotImplementedError(f"{what}: the encoder is in train mode with dropout > 0 - call eval() for attribution")
        if vit._fp8 is not None:
            raise NotImplementedError(f"{what}: not through the fp8 forwards (enable_fp8) - disable_fp8() first")
        return S, S // self.config['TRAINING_VIT_PATCH_SIZE'], T, int(chunk)

    def _head_seed(self, z, target):
        """z [B, T, 2] -> (logits [B, 2], class_idx [B], dx [B, T, 2] = d logit_class / d z): one forward and one backward launch of the
        temporal head; the parameter gradients of that backward go to a scratch arena, so no p.grad of the head is touched"""
        from . import ops
        head = self._temporal_head
        arena, _ = head.flat_parameters()
        with torch.no_grad():
            logits = ops.temporal_head_fwd(z, arena, head.ff, head.eps)
            class_idx = target_classes(target, logits)
            dx = ops.temporal_head_bwd(z, arena, head.ff, F.one_hot(class_idx, 2).to(torch.float32), torch.empty_like(arena), accumulate=False,
                                       want_dx=True, eps=head.eps)
        return logits, class_idx, dx

    def attribution_series(self, x, method="gradcam", target=None, threshold=None, scope="series", layout="series", chunk=None):
        """Spatio-temporal attribution of a batch of series x [B, H, W, D, T] (4D model): which regions drove a class at every timepoint.
        The explained class is that of the FINAL logits (temporal head and projection): target None = their arg-max, an int, or a
        LongTensor [B].  Volume (b, t) is seeded with dx[b, t, :] = d logit_class[b] / d volume_logits[b, t, :], from one backward launch of
        the temporal head (its parameter gradients go to a scratch arena):
          gradcam    the encoder's data-only backward from dlogits = dx (ViT.recording_forward / data_backward: no autograd graph, no input
                     gradient), then the Grad-CAM reduction of the taps (nv_gradcam_reduce_grouped);
          relevance  the attention relevance terms of the same backward (form "relevance"), accumulated by nv_attn_relevance;
          rollout    ViT.attention_rollout of every timepoint, as for the 3D model: class-agnostic - `target` only sets class_idx, and the
                     magnitudes it shows across time carry NO class information (they compare how peaked the attention of two timepoints is,
                     not how much either matters for the class).
        scope "series" normalises (min-max) and cuts (the top `threshold` % of the cells, None = GRADCAM_THRESHOLD) over the T G^3 cells of a
        sample jointly, so relative importance across time survives; "volume" treats every timepoint on its own, with the bits of the 3D
        path (attribution_volumes).  layout "series": volumes [B, S, S, S, T], time innermost as x and a 4D NIfTI; "frames": [B, T, S, S, S].
        chunk: volumes per encoder pass (None = 64).  With B T > chunk the volume logits of all timepoints are needed before any seed
        exists: the recording forwards run twice with the same arithmetic, the second run keeps the activations (Grad-CAM then gathers the
        taps of all chunks, 6 bytes per element of [B T, n, d]).
        "Normalised" is the reference's (v - min) / (max - min + 1e-8): a map peaks at r / (r + 1e-8) of its raw range r.  The seed passes
        the head's two-feature LayerNorms, which volume logits of order 1 saturate (~1e-11 of a gradient gets through): Grad-CAM and
        relevance maps then peak at 1e-6 .. 1e-4, in effect raw * 1e8 - the kept cells and their ranking are right, rescale by the map's
        maximum for display.
        Returns a dict of device tensors: volumes fp32; token_maps [B, T, G^3] normalised; class_idx [B]; logits [B, 2]; volume_logits
        [B, T, 2]; temporal [B, T] = sum_c dx * volume_logits (temporal_importance's grad_x_input); cuts [B] (scope "series") or [B, T].
        No p.grad is touched, it works under no_grad and needs no requires_grad on x; nothing crosses PCIe and nothing synchronises with
        the host.  Refused (NotImplementedError, before any device work): a 3D model, a temporal head the native kernel does not compute,
        head or encoder in train mode with dropout > 0, the fp8 forwards, T G^3 > 32768 with scope "series" (use scope="volume")."""
        from . import ops
        if method not in self.SERIES_METHODS:
            raise ValueError(f"attribution_series: method must be 'gradcam', 'rollout' or 'relevance', got {method!r}")
        if scope not in ops.SERIES_SCOPES:
            raise ValueError(f"attribution_series: scope must be 'series' or 'volume', got {scope!r}")
        if layout not in ops.SERIES_LAYOUTS:
            raise ValueError(f"attribution_series: layout must be 'series' or 'frames', got {layout!r}")
        S, G, T, chunk = self._series_inputs("attribution_series", x, target, chunk)
        N = G ** 3
        if scope == "series" and T * N > ops.SERIES_MAX_CELLS:
            raise NotImplementedError(f"attribution_series: {T} timepoints of {N} cells are more than the {ops.SERIES_MAX_CELLS} cells one sample may "
                                      'have under scope="series" - use scope="volume"')
        keep_percent = _grid_geometry(self.config, threshold)[2]
        vit = self.volume_encoder.vit3d
        if method != "rollout":
            vit._check_data_backward()
        series = x.detach().to(device=self.device, dtype=torch.float32)
        B = series.shape[0]
        V = B * T
        # [B, H, W, D, T] -> [B T, H, W, D] (one strided copy: the fused 4D gather is forward-only) in ViT3DEncoder.forward's view
        video = series.movedim(-1, 1).reshape(V, S, S, S).permute(0, 3, 1, 2).unsqueeze(1)
        vit.check_video(video)
        spans = [(first, min(chunk, V - first)) for first in range(0, V, chunk)]
        part = lambda first, count: video[first:first + count]

        with torch.no_grad():
            if method == "rollout":
                passes = [vit.attention_rollout(part(*span)) for span in spans]
                z = torch.cat([logits for logits, _ in passes]).view(B, T, 2)
                raw = torch.cat([maps for _, maps in passes]).view(B, T, N)
                logits, class_idx, dx = self._head_seed(z, target)
            else:
                # every seed needs the volume logits of all T timepoints of its sample
                z = torch.cat([vit.recording_forward(part(*span)) for span in spans]).view(B, T, 2)
                logits, class_idx, dx = self._head_seed(z, target)
                seeds = dx.view(V, 2)
                layers = list(range(vit._cfg.depth)) if method == "relevance" else None
                taps, rows = None, []
                for first, count in spans:
                    if len(spans) > 1:
                        vit.recording_forward(part(first, count))          # the same arithmetic again; this run's activations are kept
                    terms = vit.data_backward(seeds[first:first + count], layers, "relevance")
                    if method == "relevance":
                        rows.append(ops.attn_relevance([terms[l] for l in layers], start_mean=vit.pool == "mean"))
                        continue
                    act, grad = vit.last_attn_norm_output_raw(), vit.last_attn_norm_grad_raw()
                    if len(spans) == 1:
                        taps = (act, grad)
                    else:
                        if taps is None:
                            taps = (act.new_empty((V,) + tuple(act.shape[1:])), grad.new_empty((V,) + tuple(grad.shape[1:])))
                        taps[0][first:first + count].copy_(act)
                        taps[1][first:first + count].copy_(grad)
                if method == "relevance":
                    raw = torch.cat(rows).view(B, T, N)
                else:
                    raw = ops.gradcam_reduce_grouped(taps[0], taps[1], T if scope == "series" else 1)[0].view(B, T, N)
            volumes, (token_maps, _, cuts) = ops.series_maps_to_volumes(raw.contiguous(), G, S, normalize=method != "gradcam", scope=scope,
                                                                       keep_percent=keep_percent, layout=layout, return_maps=True)
            temporal = ops.temporal_grad_x_input(dx, z.contiguous())
        return {"volumes": volumes, "token_maps": token_maps, "class_idx": class_idx, "logits": logits, "volume_logits": z, "temporal": temporal,
                "cuts": cuts}

    def temporal_importance(self, x, target=None, baseline=0.0, score=None):
        """Which timepoints of a series x [B, H, W, D, T] drove a class of the 4D model, two ways, from ONE encoder pass over the B T
        volumes (the model's own no-grad forward: the fused no-copy 4D gather when T % 4 == 0) plus one forward of a single constant
        volume filled with `baseline` (a float):
          occlusion     [B, T] = score(z) - score(z with z[b, t] replaced by z_base): z the encoder's logits per timepoint, z_base the
                        baseline volume's; the B (T + 1) sequences (nv_series_leave_one_out) go through ONE launch of the temporal head;
                        score "prob" (softmax probability of the class) or "logit";
          grad_x_input  [B, T] = sum_c dx[b, t, c] z[b, t, c] with dx = d logit_class / d z (one backward launch of the head, parameter
                        gradients to a scratch arena).
        target: None = the arg-max of the final logits, an int, or a LongTensor [B].  Returns a dict of device tensors: occlusion,
        grad_x_input, class_idx [B], scores [B, T + 1] (column 0: the unperturbed series, column 1 + t: timepoint t replaced), logits
        [B, 2], volume_logits [B, T, 2].  Refusals and side effects (none) as attribution_series."""
        from . import ops
        score = self._resolve_score("temporal_importance", score)
        if score not in ops.SCORE_KINDS:
            raise ValueError(f"temporal_importance: score must be 'prob' or 'logit', got {score!r}")
        if torch.is_tensor(baseline) or isinstance(baseline, bool) or not isinstance(baseline, (int, float)):
            raise ValueError(f"temporal_importance: baseline must be a float (one constant volume), got {type(baseline).__name__}")
        S, _, T, _ = self._series_inputs("temporal_importance", x, target, None)
        series = x.detach().to(device=self.device, dtype=torch.float32)
        B, device = series.shape[0], series.device
        head = self._temporal_head
        arena, _ = head.flat_parameters()

        def build():
            b = torch.arange(B, device=device, dtype=torch.int64).repeat_interleave(T + 1)
            return torch.stack([b, torch.zeros_like(b), torch.zeros_like(b)], 1).to(torch.int32).contiguous()
        jobs = cached_table(self, "_perturbation_tables", ("temporal", str(device), B, T), build)

        with torch.no_grad():
            z = self._volume_logits(series).float().contiguous()
            z_base = self.volume_encoder(torch.full((1, S, S, S), float(baseline), dtype=torch.float32, device=device))[0].float().contiguous()
            logits, class_idx, dx = self._head_seed(z, target)
            out = ops.temporal_head_fwd(ops.series_leave_one_out(z, z_base), arena, head.ff, head.eps)
            scores = ops.class_scores(out, jobs, class_idx, kind=score).view(B, T + 1)
            occlusion = scores[:, :1] - scores[:, 1:]
            grad_x_input = ops.temporal_grad_x_input(dx, z)
        return {"occlusion": occlusion, "grad_x_input": grad_x_input, "class_idx": class_idx, "scores": scores, "logits": logits, "volume_logits": z}

    def visualize_slice(self, cam_3d, original_volume):
        """One 2-D slice of the volume and of its CAM along GRADCAM_SLICE_DIM at GRADCAM_SLICE_IDX
        (contract of NeuroEncoder.py:135-168: returns (img, attn), or None after printing why not)."""
        axis, index = self.config['GRADCAM_SLICE_DIM'], self.config['GRADCAM_SLICE_IDX']
        if cam_3d is None:
            print("Error: No CAM computed")
            return None
        volume = original_volume.squeeze().detach().cpu().numpy()
        if volume.ndim != 3 or cam_3d.ndim != 3:
            print(f"Shape mismatch: original {volume.shape}, CAM {cam_3d.shape}")
            return None
        if axis not in (0, 1, 2):
            print(f"Invalid slice dimension: {axis}")
            return None
        pick = tuple(index if a == axis else slice(None) for a in range(3))
        return volume[pick], cam_3d[pick]


class _NeuroEncoderTwin(NeuroEncoder):
    """NeuroEncoder(config) that reads no file: the 4D model's encoder is frozen as ever, its weights arrive with the load_state_dict
    that twin_of does next."""

    def _adopt_trained_encoder(self, checkpoint_path: str) -> None:
        self.volume_encoder.requires_grad_(False)
        self.volume_encoder.eval()


def twin_of(model: NeuroEncoder) -> NeuroEncoder:
    """A second NeuroEncoder of `model`'s config holding a copy of its parameters (optim.ModelEma's averaged model): built from the
    config plus load_state_dict - engine.VitRuntime owns workspaces, streams and events that a deep copy must not share - with the
    encoder's operand format, eval precision and LayerNorm-fold switch carried over.  `model` is not touched, no checkpoint is read
    again, and torch's CPU generator is left where it was (the construction draws an initialisation that is overwritten at once)."""
    with torch.random.fork_rng(devices=[]):
        twin = _NeuroEncoderTwin(model.config)
    src, dst = model.volume_encoder.vit3d, twin.volume_encoder.vit3d
    dst.set_operands(src.operands)
    dst.eval_precision, dst.fold_layernorm = src.eval_precision, src.fold_layernorm
    twin.load_state_dict(model.state_dict(), strict=True)
    return twin


class ViT3DEncoder(nn.Module):
    """NeuroEncoder.py:171-205: config -> ViT, and the [B,H,W,D] -> [B,1,D,H,W] input view."""

    # the transformer size the reference hard-codes (NeuroEncoder.py:187-190); optional TRAINING_VIT_* keys override it
    REFERENCE_SIZE = {'TRAINING_VIT_DIM': 1024, 'TRAINING_VIT_DEPTH': 6, 'TRAINING_VIT_HEADS': 8, 'TRAINING_VIT_DIM_HEAD': 64,
                      'TRAINING_VIT_MLP_DIM': 2048}

    def __init__(self, config):
        super().__init__()
        self.device = config['DEVICE']
        self.dropout = config['TRAINING_DROPOUT']
        self.grid_size = config['TRAINING_VIT_INPUT_SIZE']
        self.cube_size = config['GRADCAM_CUBE_SIZE']
        self.patch_size = config['TRAINING_VIT_PATCH_SIZE']
        size = {key: config.get(key, default) for key, default in self.REFERENCE_SIZE.items()}
        # the synthetic cube-localisation task has one class per cube position (NeuroEncoder.py:179); everything else is binary
        cubes_per_axis = self.grid_size // self.cube_size
        classes = cubes_per_axis ** 3 if config['DATASET_NAME'] == 'gradcam' else 2
        # TRAINING_OBJECTIVE "regression" (optional key): the head predicts REGRESSION_TARGETS (default 1) continuous targets on the scale
        # standardised by REGRESSION_TARGET_MEAN / _STD (lists of that many numbers, default 0 / 1) - non-persistent buffers: the
        # state_dict keys stay the reference's
        self.regression = config.get('TRAINING_OBJECTIVE', None) == "regression"
        if self.regression:
            if config['TRAINING_DIM'] == 4:
                raise NotImplementedError("TRAINING_OBJECTIVE 'regression' is for the 3D model - the 4D model's temporal head is built around two features")
            classes = self._regression_scale(config)
        # a cubic single-channel volume: frames (depth) and image sides share one extent and one patch edge
        # stochastic depth (timm's drop_path_rate, linear over the blocks; 0.1 in the DeiT-B / MAE fine-tuning recipes): optional key, absent = 0
        self.drop_path = config.get('TRAINING_DROP_PATH', 0.0)
        if config['TRAINING_DIM'] == 4 and self.drop_path:
            raise NotImplementedError("TRAINING_DROP_PATH: stochastic depth is for the 3D model - the 4D model's encoder is frozen and kept in eval mode")
        self.vit3d = ViT(image_size=self.grid_size, image_patch_size=self.patch_size, frames=self.grid_size, frame_patch_size=self.patch_size,
                         channels=1, num_classes=classes, dim=size['TRAINING_VIT_DIM'], depth=size['TRAINING_VIT_DEPTH'],
                         heads=size['TRAINING_VIT_HEADS'], dim_head=size['TRAINING_VIT_DIM_HEAD'], mlp_dim=size['TRAINING_VIT_MLP_DIM'],
                         pool='cls', dropout=self.dropout, emb_dropout=self.dropout, drop_path_rate=self.drop_path).to(self.device)
        # arithmetic of eval-mode no-grad forwards: "bf16" (default; the training arithmetic) or "fp32" (the reference's validate,
        # Trainer.py:101-118).  The Trainer shell's validate / evaluate_samples use VALIDATION_PRECISION (default "fp32").
        self.vit3d.eval_precision = config.get('TRAINING_VIT_EVAL_PRECISION', 'bf16')
        # 16-bit MFMA operand format of the training arithmetic: "bf16" (default) or "fp16" - what the reference's autocast(float16)
        # computes in (Trainer.py:68); TrainStep then scales the loss as its GradScaler does (Trainer.py:29,74-76)
        self.vit3d.set_operands(config.get('TRAINING_VIT_OPERANDS', 'bf16'))

    def _regression_scale(self, config) -> int:
        """REGRESSION_TARGETS, checked, and the buffers target_mean / target_std [K] of the raw scale"""
        K = config.get('REGRESSION_TARGETS', 1)
        if isinstance(K, bool) or not isinstance(K, int) or K < 1:
            raise ValueError(f"REGRESSION_TARGETS must be a positive integer, got {K!r}")
        for key, name, default in (('REGRESSION_TARGET_MEAN', 'target_mean', 0.0), ('REGRESSION_TARGET_STD', 'target_std', 1.0)):
            given = config.get(key, None)
            given = [default] * K if given is None else ([given] if isinstance(given, (int, float)) else list(given))
            t = torch.tensor([float(g) for g in given], dtype=torch.float32)
            if t.numel() != K or not bool(torch.isfinite(t).all()) or (name == 'target_std' and not bool((t > 0).all())):
                raise ValueError(f"{key} must be {K} finite numbers" + (" > 0" if name == 'target_std' else "") + f", got {given!r}")
            self.register_buffer(name, t, persistent=False)
        return K

    def forward_raw(self, raw, crop=None):
        from .preprocess import ADNI_CROP, crop_view, volume_sigma
        crop = ADNI_CROP if crop is None else crop
        raw = raw.to(self.device)
        if raw.dtype != torch.float32:                                 # int16 scanner data: the gather kernel reads float32 -> separate pass
            from .preprocess import zscore_crop
            return self.forward(zscore_crop(raw, crop))
        sigma = volume_sigma(raw, crop)                                # std + 1e-8 per cropped volume (statistics in double)
        view = crop_view(raw, crop)                                    # [B, Sx, Sy, Sz] strided view of the raw tensor
        return self.vit3d(view.permute(0, 3, 1, 2).unsqueeze(1), vol_sigma=sigma)

    def forward(self, x):
        # x: (batch, H, W, D).  The permuted tensor is only a VIEW: the patch-gather kernel reads the original
        # [B,H,W,D] memory through its strides, so the reference's permute never costs a copy.
        volume = x.to(self.device)
        return self.vit3d(volume.permute(0, 3, 1, 2).unsqueeze(1))      # (batch, channel = 1, frames = D, height = H, width = W)


class TemporalTransformer(nn.Module):
    """NeuroEncoder.py:207-217.  d_model = 2 (the frozen ViT3D emits 2 logits): 10 274 parameters.  The stock module is the
    parameter holder (reference state_dict keys and initialisation); NeuroEncoder.forward computes it through temporal.TemporalHead."""

    D_MODEL, HEADS, LAYERS = 2, 2, 1      # NeuroEncoder.py:210-211: the sequence elements are the encoder's two logits

    def __init__(self, config):
        super().__init__()
        self.device = config['DEVICE']
        block = nn.TransformerEncoderLayer(d_model=self.D_MODEL, nhead=self.HEADS, batch_first=True)
        self.transformer = nn.TransformerEncoder(block, num_layers=self.LAYERS).to(self.device)

    def forward(self, x):
        return self.transformer(x)


class ProjectionHead(nn.Module):
    """NeuroEncoder.py:219-230."""

    def __init__(self, config):
        super().__init__()
        self.device = config['DEVICE']
        self.projection_head = nn.Linear(2, 2).to(self.device)

    def forward(self, x):
        return self.projection_head(x)
