"""MLD -- the orchestration class of the path, with the method surface of
``mld.models.modeltype.mld.MLD`` / ``base.BaseModel`` (reference mld.py:88-2130, base.py:38-213) but
without Lightning: ``training_step / validation_step / test_step / allsplit_step``,
``_diffusion_reverse``, ``_diffusion_process``, ``train_diffusion_forward``, ``train_vae_forward``,
``ego_eval``, ``forward`` / ``sample``, ``configure_optimizers``.

What runs where
  * VAE encode/decode, the whole reverse-diffusion loop, the denoiser forward, PointNet, SMPL, rotation
    helpers and renorm run in libseeme_hip.so (HIP kernels for gfx950).
  * Stage-2 *training*: the frozen encoders and the denoiser forward + hand-written backward
    (``denoiser_train.py``: ``k_den_sample`` with saves, ``k_den_bwd``, ``seeme_den_wgrad``) are HIP; the table builders
    around the chain (rsample, add_noise, time MLP, output_scene, condition / time tables) are hand-written too
    (``stage2_glue.py``: one autograd node for the whole step); every gradient lives in one flat buffer
    (``distributed.GradBucket``) that is all-reduced in place and consumed by the one-launch AdamW.  More than one
    attention head falls back to the autograd twin (``denoiser_autograd.py``).
  * Stage-1 (VAE) *training*: hand-written HIP forward-with-saves / backward of the encoder and the decoder
    (``vae_train.py``: grouped fp32 GEMMs + LayerNorm / softmax / GELU / dropout kernels) and of the SMPL joint regressor
    (``smpl._JointsAA``); the differentiable twins (``vae_autograd.py``) are the fallback; evaluation of that stage is HIP.
  * Only the live flows are implemented; the reference's dead code (``forward`` calling the undefined
    ``feats2joints``, t2m_eval, the ``save_for_edo`` debug dump -- SURVEY.md App. D) is not reproduced:
    ``forward``/``sample`` = what ``ego_eval`` really does (condition -> reverse diffusion -> decode).
  * Sampling is one set of steps with three callers (``ego_eval`` at K = 1, ``_ego_eval_hypotheses`` for K > 1, ``predict``):
    ``_condition_tokens`` -> ``_posterior_draws`` / ``_condition_rows`` -> ``_diffusion_reverse`` (one launch) or
    ``_diffusion_reverse_rows`` (at most 512 rows per launch) -> one decode or ``_decode_rows``.
  * The image condition takes the ResNet-50 backbone's pooled features [B,2048] in the batch's image slot or, with
    ``model.image_backbone``, the crops themselves (the backbone then runs here, frozen and in eval mode: seeme_amd/resnet.py);
    ``output_images`` is trainable and its stage-2 forward / gradient are glue problems, evaluation projects with a torch op.
  * Deliberate, documented deviations from the reference: none by default, except where the reference cannot
    run as written (the image branches of ``ego_eval``: batch layout, guidance).  ``TEST.SAMPLE_MEAN``
    (condition on the posterior mean instead of a sample) and ``TEST.CFG_SCENE_ORDER: fixed`` (classifier-free guidance
    with the unconditional scene token in the unconditional half) are opt-in.
"""
from __future__ import annotations

import contextlib

import inspect
import time
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import geometry as G
from .config import instantiate_from_config
from .denoiser_autograd import denoiser_forward_torch
from .hyp_metrics import (K_MAX, HypothesisMetrics, SelectionMetrics, best_index, check_select, hyp_metrics_hip, hyp_pairdist_hip,
                          keep_mask, select_index)
from .mesh_metrics import COLLISION_HYP, COLLISION_REF, CollisionMetrics, MeshMetrics, check_closed_faces, mesh_metrics_eval
from .resnet import ResNet50
from .recording import check_head_offset
from .respointnet import ResnetPointnet
from .shapes import motion_layout
from .smpl import SMPL
from .social_metrics import DEFAULT_DIST_EDGES, DEFAULT_GAZE_EDGES, SocialMetrics, check_edges, social_metrics_hip
from .track import DEFAULT_PRIOR_WEIGHT, DEFAULT_SIGMA, DEFAULT_STEP_MM, check_prior_weight, check_sigma, check_step_mm


IMAGE_FEAT_DIM = 2048          # pooled ResNet-50 feature of proscene.encode_image (prohmr_scene.py:99-100, BACKBONE.OUT_CHANNELS)


def split_batch(condition, batch):
    """The dataset's tuple by condition (dataset.py:1754-1794): (motion, transl, beta, utils, scene | None, images | None, length,
    rest).  image + scene: (..., scene, images, length); image only: (..., images, length); scene only: (..., scene, length,
    names | interactee ground truth); neither: (..., length)."""
    motion, transl, beta, utils_ = batch[:4]
    k = 4
    scene = images = None
    if "scene" in condition:
        scene, k = batch[k], k + 1
    if "image" in condition:
        images, k = batch[k], k + 1
    return motion, transl, beta, utils_, scene, images, batch[k], tuple(batch[k + 1:])


# ----------------------------------------------------------------------------- losses / metrics
_WARNED = set()


def _warn_once(key: str, msg: str) -> None:
    """Fallbacks onto the autograd twins are announced once per process (they used to be silent)."""
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


class MLDLosses:
    """mld/models/losses/mld.py:10-176 without torchmetrics: running sums + the weighted total."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.stage = cfg.TRAIN.STAGE
        self.predict_epsilon = cfg.TRAIN.ABLATION.PREDICT_EPSILON
        self.predict_transl = cfg.TRAIN.ABLATION.PREDICT_TRANSL
        if self.stage not in ("vae", "diffusion", "vae_diffusion"):
            raise ValueError(f"Stage {self.stage} not supported")
        self.sums: Dict[str, float] = {}
        self.count = 0
        self.accumulate = True

    def _acc(self, name, val, weight):
        if self.accumulate:    # running sums stay on the device: no host sync per step (compute() converts)
            self.sums[name] = self.sums.get(name, 0.0) + val.detach()
        return weight * val

    @staticmethod
    def align_root(gt, pred):
        pg, pp = gt[:, :, [0]], pred[:, :, [0]]
        return gt - pg, pred - pp, pg, pp

    def update(self, rs, accumulate: bool = True):
        self.accumulate = accumulate
        L = self.cfg.LOSS
        total = 0.0
        mse = nn.functional.mse_loss
        sl1 = nn.functional.smooth_l1_loss
        if self.stage in ("vae", "vae_diffusion"):
            jr, jp = rs["joints_ref"], rs["joints_rst"]
            if self.predict_transl:
                jr, jp, pg, pp = self.align_root(jr, jp)
                # weight: the reference's elif chain tests split('_')[0] == 'recons' before 'transl' (losses/mld.py:80-97),
                # so recons_transl is weighted by LAMBDA_REC and its LAMBDA_ROOT branch is unreachable
                total = total + self._acc("recons_transl", sl1(pp, pg), L.LAMBDA_REC)
            total = total + self._acc("recons_feature", sl1(rs["m_rst"], rs["m_ref"]), L.LAMBDA_REC)
            total = total + self._acc("recons_joints", sl1(jp, jr), L.get("LAMBDA_JOINT", 1.0))
            if L.LAMBDA_KL != 0.0:
                kl = torch.distributions.kl_divergence(rs["dist_m"], rs["dist_ref"]).mean()
                total = total + self._acc("kl_motion", kl, L.LAMBDA_KL)
        if self.stage in ("diffusion", "vae_diffusion"):
            if self.predict_epsilon:
                total = total + self._acc("inst_loss", mse(rs["noise_pred"], rs["noise"]), 1.0)
            else:
                total = total + self._acc("x_loss", mse(rs["pred"], rs["latent"]), 1.0)
        if accumulate:
            self.sums["total"] = self.sums.get("total", 0.0) + total.detach()
            self.count += 1
        return total

    def compute(self):
        return {k: float(v) / max(self.count, 1) for k, v in self.sums.items()}

    def reset(self):
        self.sums, self.count = {}, 0


class EgoMetrics:
    """ComputeMetrics of the reference (metrics/compute.py:349-580,184-232) on the device, without its per-sequence
    `.cpu().numpy()` loops: MPJPE and root error after first-frame head (joint 15) and per-frame pelvis alignment
    (:364-399,470-473), acceleration error (:243-271,474) and head-orientation error ||I - R_gt R_pred^-1||_F
    (:338-346,469), x1000 where the reference does; per-sequence means averaged over the sequences the reference
    counts: on 'test' only those with head error < 0.9, root error < 300 mm and a non-zero acceleration error
    (:488-517), otherwise those with a non-zero acceleration error (:567-576).  Sums are one device tensor, so
    the multi-GPU reduction is one small all-reduce (seeme_amd.distributed.reduce_sums)."""

    NAMES = ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR", "mpjpe_interactee")

    def __init__(self):
        self.reset()

    def reset(self):
        self._sums = None            # [5 sums, 5 counts] float64 on the device of the first update

    @staticmethod
    def quat_to_rotmat(q):
        """(w,x,y,z) -> [M,3,3], normalising as transformations.quaternion_matrix does (compute.py:292)."""
        n = (q * q).sum(-1, keepdim=True)
        q = q * torch.sqrt(2.0 / n.clamp_min(1e-30))
        w, x, y, z = q.unbind(-1)
        R = torch.stack([1 - y * y - z * z, x * y - z * w, x * z + y * w,
                         x * y + z * w, 1 - x * x - z * z, y * z - x * w,
                         x * z - y * w, y * z + x * w, 1 - x * x - y * y], dim=-1).reshape(-1, 3, 3)
        return torch.where((n < 1e-15)[..., None], torch.eye(3, device=q.device, dtype=q.dtype).expand_as(R), R)

    @staticmethod
    def per_sequence(jts_pred, jts_ref, lengths, quat_pred=None, quat_ref=None):
        B, T = jts_ref.shape[:2]
        dev = jts_ref.device
        ref = jts_ref - jts_ref[:, 0:1, 15:16, :]
        pred = jts_pred - jts_pred[:, 0:1, 15:16, :]
        pelvis_ref, pelvis_pred = ref[:, :, [0]], pred[:, :, [0]]
        ref, pred = ref - pelvis_ref, pred - pelvis_pred
        lens = torch.as_tensor(lengths, device=dev).reshape(B)
        frame = torch.arange(T, device=dev)[None, :]
        mask = (frame < lens[:, None]).to(ref.dtype)
        out = {}
        out["MPJPE"] = ((pred - ref).norm(dim=-1).mean(dim=-1) * mask).sum(1) / lens * 1000.0
        out["ROOT_ERROR"] = ((pelvis_pred - pelvis_ref).norm(dim=-1).squeeze(-1) * mask).sum(1) / lens * 1000.0
        if T >= 3:   # X[t-1] - 2 X[t] + X[t+1] over the valid frames (compute.py:257-271)
            acc = lambda x: x[:, :-2] - 2 * x[:, 1:-1] + x[:, 2:]
            amask = (frame[:, : T - 2] < (lens - 2)[:, None]).to(ref.dtype)
            an = (acc(pred) - acc(ref)).norm(dim=-1).mean(dim=-1)
            out["ACCL"] = (an * amask).sum(1) / (lens - 2).clamp_min(1) * 1000.0
        else:
            out["ACCL"] = torch.zeros(B, device=dev, dtype=ref.dtype)
        if quat_pred is not None and quat_ref is not None:
            out["HEAD_ORIENTATION_ERROR"] = EgoMetrics.head_orientation_error(quat_pred, quat_ref, mask, lens)
        else:
            out["HEAD_ORIENTATION_ERROR"] = torch.zeros(B, device=dev, dtype=ref.dtype)
        return out

    @staticmethod
    def head_orientation_error(quat_pred, quat_ref, mask, lens):
        """||I - R_gt R_pred^-1||_F per frame (compute.py:338-346), mean over the valid frames; quaternions [M*T,4], mask [M,T]."""
        M, T = mask.shape
        Rg = EgoMetrics.quat_to_rotmat(quat_ref.reshape(-1, 4).to(mask.dtype))
        Rp = EgoMetrics.quat_to_rotmat(quat_pred.reshape(-1, 4).to(mask.dtype))
        err = (torch.eye(3, device=mask.device, dtype=mask.dtype) - Rg @ torch.linalg.inv(Rp)).flatten(1).norm(dim=1).reshape(M, T)
        return (err * mask).sum(1) / lens

    def update(self, jts_pred, jts_ref, lengths, quat_pred=None, quat_ref=None, split: str = "test",
               jts_int=None, jts_int_gt=None):
        m = self.per_sequence(jts_pred, jts_ref, lengths, quat_pred, quat_ref)
        every = torch.ones_like(m["MPJPE"], dtype=torch.bool)
        if jts_int is not None and jts_int_gt is not None:      # POSE_ESTIMATION_TASK: every sequence counts (compute.py:476-481)
            a, g = jts_int - jts_int[:, :, [0]], jts_int_gt - jts_int_gt[:, :, [0]]
            T = a.shape[1]
            lens = torch.as_tensor(lengths, device=a.device).reshape(-1)
            mask = (torch.arange(T, device=a.device)[None, :] < lens[:, None]).to(a.dtype)
            m["mpjpe_interactee"] = ((a - g).norm(dim=-1).mean(dim=-1) * mask).sum(1) / lens * 1000.0
        else:
            m["mpjpe_interactee"] = torch.zeros_like(m["MPJPE"])
            every = ~every
        moving = m["ACCL"] > 0
        have_q = quat_pred is not None and quat_ref is not None
        if split == "test" and have_q:
            keep = moving & (m["HEAD_ORIENTATION_ERROR"] < 0.9) & (m["ROOT_ERROR"] < 300.0)
            cols = (keep, keep, keep, keep, every)
        else:                        # train / val: MPJPE and root error only (compute.py:567-576)
            none = torch.zeros_like(moving)
            cols = (moving, moving, none, none, every) if split != "test" else (moving, moving, moving, none, every)
        vals = torch.stack([(m[k] * c).sum() for k, c in zip(self.NAMES, cols)] + [c.sum().to(m["MPJPE"].dtype) for c in cols]).double()
        self._sums = vals if self._sums is None else self._sums + vals

    def sums(self):
        return torch.zeros(2 * len(self.NAMES), dtype=torch.float64) if self._sums is None else self._sums

    def compute(self, sums=None):
        s = (self.sums() if sums is None else sums).detach().double().cpu()
        n = len(self.NAMES)
        return {k: float(s[i]) / max(float(s[n + i]), 1.0) for i, k in enumerate(self.NAMES)} | {"count_seq": float(s[n])}


class SyntheticEgoDataModule:
    """Batches with the EgoBody/GIMO tuple layout (mld/data/humanml/data/dataset.py:1754-1794, 2479-2509): motion
    [B,T,2,72 | 66], transl [B,2,T,3], beta [B,2,T,10], utils [B,T,6], scene [B,P,3], length [B,1]; mean/std
    for ``renorm`` (mld/data/EgoBody.py:151-157).  Datasets are licence-gated, so this is what tests and
    benchmarks run on.

    data_type "rot6d" (EgoBody only, nfeats 144): motion [B,T,2,144] whose RENORMED values are the rot6d encoding of random
    rotations -- axis-angle draws -> rotation matrices -> the first two columns in the order the model reads
    (``geometry.rot6d_to_rotmat``'s default), then the inverse of ``renorm`` -- so that training on these batches stays away from
    degenerate Gram-Schmidt inputs; the translation stays raw and outside the features."""

    def __init__(self, nfeats=75, T=196, n_points=2048, seed=1234, device="cpu", pose_dim=None, data_type="angle"):
        if data_type not in ("angle", "rot6d"):
            raise ValueError(f"data_type must be 'angle' or 'rot6d', got {data_type!r}")
        self.data_type = data_type
        if data_type == "rot6d":
            if nfeats != 144 or pose_dim not in (None, 144):
                raise ValueError(f"data_type 'rot6d' is 24 joints x 6 = 144 features (nfeats {nfeats}, pose_dim {pose_dim})")
            pose_dim = 144
        self.nfeats, self.T, self.n_points = nfeats, T, n_points
        # per-person pose width of `motion`: EgoBody 72 (24 joints, axis-angle), GIMO 66 (root + 21 joints); the VAE sees
        # pose + 3 translation values = nfeats when TRAIN.ABLATION.PREDICT_TRANSL (mld.py:121-123)
        self.pose_dim = int(pose_dim) if pose_dim is not None else nfeats - 3
        g = torch.Generator().manual_seed(seed)
        self.mean = (0.1 * torch.randn(1, nfeats + 16, generator=g)).to(device)
        self.std = (0.5 + torch.rand(1, nfeats + 16, generator=g)).to(device)
        self.device = device
        self.is_mm = False
        self.seed = seed

    def renorm(self, features):
        return G.renorm(features, self.mean, self.std)

    def batch(self, B, idx=0, with_scene=False, lengths=None, pose_estimation=False, split="train", with_image=False):
        """with_image: pooled image features [B,2048] (non-negative, as after the backbone's final ReLU + pooling) in the image
        layouts (motion, transl, beta, utils, [scene], images, length); with_image="crops": seeded smooth uint8 crops
        [B,224,224,3] instead (what EgoDataModule hands over with the backbone on)."""
        g = torch.Generator().manual_seed(self.seed * 7919 + idx)
        T = self.T
        rot6d = self.data_type == "rot6d"
        motion = 0.5 * torch.randn(B, T, 2, 72 if rot6d else self.pose_dim, generator=g)
        if rot6d:
            aa, motion = motion, self._encode_rot6d(motion)
        transl = torch.randn(B, 2, T, 3, generator=g)
        beta = 0.5 * torch.randn(B, 2, 1, 10, generator=g).expand(B, 2, T, 10).contiguous()
        utils_ = torch.zeros(B, T, 6)
        length = torch.full((B, 1), T, dtype=torch.long) if lengths is None else torch.as_tensor(lengths).reshape(B, 1)
        dev = self.device
        out = [motion.to(dev), transl.to(dev), beta.to(dev), utils_.to(dev)]
        if with_scene:
            out.append((torch.rand(B, self.n_points, 3, generator=g) * 6 - 3).to(dev))
        if with_image:
            if pose_estimation:
                raise NotImplementedError("the image layouts carry no interactee ground truth (dataset.py:1788-1792)")
            # (a generator of its own: the other tensors stay those of the same idx without images)
            gi = torch.Generator().manual_seed(self.seed * 7919 + idx + 104729)
            if isinstance(with_image, str):
                if with_image != "crops":
                    raise ValueError("with_image: False, True (pooled features) or 'crops' (uint8 crops)")
                # bilinear upsampling of 7x7 uniform noise: smooth, full 0..255 range
                low = torch.rand(B, 3, 7, 7, generator=gi)
                up = torch.nn.functional.interpolate(low, size=(224, 224), mode="bilinear", align_corners=False)
                out.append((up * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev))
            else:
                out.append(torch.rand(B, IMAGE_FEAT_DIM, generator=gi).pow(2).to(dev))
            out.append(length.to(dev))
            return tuple(out)
        out.append(length.to(dev))
        if with_scene and not pose_estimation:
            out.append([])          # img_path / dict_images slot
        if pose_estimation:         # interactee ground truth: motion [B,T,1,72], transl [B,1,T,3], beta [B,T,1,10] (mld.py:1119-1131)
            if rot6d:
                gt = self._encode_rot6d(aa[:, :, 1] + 0.05 * torch.randn(B, T, 72, generator=g))
            else:
                gt = motion[:, :, 1] + 0.05 * torch.randn(B, T, self.pose_dim, generator=g)
            out += [gt.unsqueeze(2).to(dev), transl[:, 1:2].clone().to(dev), beta[:, 1].unsqueeze(2).to(dev)]
        return tuple(out)

    def _encode_rot6d(self, aa):
        """axis-angle [..., 72] (CPU) -> normalised rot6d features [..., 144]: (encoding - mean) / std, the inverse of renorm."""
        r6 = G.rotmat_to_rot6d(G.aa_to_rotmat_torch(aa.reshape(-1, 3)), "prohmr").reshape(*aa.shape[:-1], 144)
        return (r6 - self.mean[0, :144].cpu()) / self.std[0, :144].cpu()


# ----------------------------------------------------------------------------- the model
class _SceneEncoderHolder(nn.Module):
    """``proscene`` -- the sub-modules of ProHMRScene on the path: ``scene_enc`` (prohmr_scene.py:102-104) for a scene condition and,
    with ``model.image_backbone``, the ResNet-50 ``backbone`` (prohmr_scene.py:33-34, 99-100) for an image condition."""

    def __init__(self, scene: bool = True, backbone: bool = False, flow: bool = False):
        super().__init__()
        if scene:
            self.scene_enc = ResnetPointnet(512, 256)
        if backbone:
            self.backbone = ResNet50()
        if flow:                                    # model.interactee_head: the pose head SMPLFlow (prohmr_scene.py:36-39)
            from .prohmr_head import SMPLFlowHead
            self.flow = SMPLFlowHead()

    def encode_scene(self, scene):
        return self.scene_enc(scene)

    def encode_image(self, images):
        return self.backbone(images)


class MLD(nn.Module):

    def __init__(self, cfg, datamodule=None, smpl_model: Optional[nn.Module] = None, **kwargs):
        super().__init__()
        self.cfg = cfg
        self.stage = cfg.TRAIN.STAGE
        self.condition = cfg.model.condition
        self.is_vae = cfg.model.vae
        self.predict_epsilon = cfg.TRAIN.ABLATION.PREDICT_EPSILON
        self.name_dataset = cfg.DATASET_NAME
        self.latent_dim = cfg.model.latent_dim
        self.guidance_scale = cfg.model.guidance_scale
        self.guidance_uncodp = cfg.model.guidance_uncondp
        self.datamodule = datamodule
        self.estimate = cfg.ESTIMATE
        self.predict_transl = cfg.TRAIN.ABLATION.PREDICT_TRANSL
        self.data_type = cfg.DATA_TYPE
        self.see_future = cfg.TEST.get("SEE_FUTURE", False)
        self.pred_global_orient = cfg.TEST.get("GLOBAL_ORIENT_PRED", True)           # mld.py:111
        # reference behaviour by default: the interactee condition is a SAMPLE of the posterior (mld.py:1280) and the CFG
        # scene pair is concatenated [cond, uncond] (mld.py:1144-1158) although _diffusion_reverse reads [uncond, cond]
        self.sample_mean = bool(cfg.TEST.get("SAMPLE_MEAN", False))
        self.cfg_scene_order = str(cfg.TEST.get("CFG_SCENE_ORDER", "reference"))
        if self.cfg_scene_order not in ("reference", "fixed"):
            raise ValueError("TEST.CFG_SCENE_ORDER must be 'reference' or 'fixed'")
        # hypotheses per sequence in ONE evaluation pass (condition encoded once, errors and diversity per sequence): 1 = today's path
        self.num_hypotheses = self._check_num_hypotheses(cfg.TEST.get("NUM_HYPOTHESES", 1), "TEST.NUM_HYPOTHESES")
        # which of the K > 1 hypotheses stands for its sequence in the keys of a K = 1 result: 'first' (hypothesis 0, today's result) or
        # 'medoid' (smallest total distance to the other draws: seeme_hyp_pairdist; needs no ground truth)
        self.hyp_select = check_select(cfg.TEST.get("HYP_SELECT", "first"), "TEST.HYP_SELECT")
        # a whole recording (predict_recording): frames shared by neighbouring windows (None: T // 4 of the batch) and the weight of
        # the medoid term against the seam term when ONE hypothesis per window is chosen (0: seams only)
        self.window_overlap = cfg.TEST.get("WINDOW_OVERLAP", None)
        if self.window_overlap is not None and (isinstance(self.window_overlap, bool) or not isinstance(self.window_overlap, int)
                                                or self.window_overlap < 0):
            raise ValueError(f"TEST.WINDOW_OVERLAP must be an integer >= 0 (at most half the window), got {self.window_overlap!r}")
        # rows of a window's scene view when a recording brings the scene's vertices and a camera pose per frame (recording.py)
        self.scene_view_points = cfg.TEST.get("SCENE_VIEW_POINTS", 20000)
        if isinstance(self.scene_view_points, bool) or not isinstance(self.scene_view_points, int) \
                or not 1 <= self.scene_view_points <= 1 << 20:
            raise ValueError(f"TEST.SCENE_VIEW_POINTS must be an integer in 1..2^20, got {self.scene_view_points!r}")
        self.path_medoid_weight = cfg.TEST.get("PATH_MEDOID_WEIGHT", 1.0)
        if isinstance(self.path_medoid_weight, bool) or not isinstance(self.path_medoid_weight, (int, float)) \
                or not 0 <= self.path_medoid_weight < float("inf"):
            raise ValueError(f"TEST.PATH_MEDOID_WEIGHT must be a finite number >= 0, got {self.path_medoid_weight!r}")
        # the headset's own path (predict_recording with head_path): the weight of the head-path term of the unary (0: off), whether
        # the stitched motion is shifted onto the path, and the Gaussian width of that shift's filter (frames; a choice, not tuned)
        self.path_head_weight = cfg.TEST.get("PATH_HEAD_WEIGHT", 0.0)
        if isinstance(self.path_head_weight, bool) or not isinstance(self.path_head_weight, (int, float)) \
                or not 0 <= self.path_head_weight < float("inf"):
            raise ValueError(f"TEST.PATH_HEAD_WEIGHT must be a finite number >= 0, got {self.path_head_weight!r}")
        self.head_anchor = cfg.TEST.get("HEAD_ANCHOR", False)
        if not isinstance(self.head_anchor, bool):
            raise ValueError(f"TEST.HEAD_ANCHOR must be true or false, got {self.head_anchor!r}")
        self.head_anchor_sigma = check_sigma(cfg.TEST.get("HEAD_ANCHOR_SIGMA", DEFAULT_SIGMA), "TEST.HEAD_ANCHOR_SIGMA")
        # the headset's orientation (predict_recording with head_rot): the weight of the head-rotation term of the unary (mm per degree;
        # 0: off; no value has been measured on data), whether the stitched motion's deviation per frame is reported, and the vector
        # from joint 15 to the device in the device's frame (metres; zeros: the device's path is taken as the joint's)
        self.path_head_rot_weight = cfg.TEST.get("PATH_HEAD_ROT_WEIGHT", 0.0)
        if isinstance(self.path_head_rot_weight, bool) or not isinstance(self.path_head_rot_weight, (int, float)) \
                or not 0 <= self.path_head_rot_weight < float("inf"):
            raise ValueError(f"TEST.PATH_HEAD_ROT_WEIGHT must be a finite number >= 0, got {self.path_head_rot_weight!r}")
        self.head_rot_report = cfg.TEST.get("HEAD_ROT_REPORT", False)
        if not isinstance(self.head_rot_report, bool):
            raise ValueError(f"TEST.HEAD_ROT_REPORT must be true or false, got {self.head_rot_report!r}")
        self.head_device_offset = check_head_offset(cfg.TEST.get("HEAD_DEVICE_OFFSET", (0.0, 0.0, 0.0)), "TEST.HEAD_DEVICE_OFFSET")
        # the body against the scene (predict_recording with scene_cloud): the weight of the body-scene term of the unary (0: off),
        # whether the stitched motion's depth per frame is reported, and the quantile of the default capsules' radii
        self.path_scene_weight = cfg.TEST.get("PATH_SCENE_WEIGHT", 0.0)
        if isinstance(self.path_scene_weight, bool) or not isinstance(self.path_scene_weight, (int, float)) \
                or not 0 <= self.path_scene_weight < float("inf"):
            raise ValueError(f"TEST.PATH_SCENE_WEIGHT must be a finite number >= 0, got {self.path_scene_weight!r}")
        self.scene_report = cfg.TEST.get("SCENE_REPORT", False)
        if not isinstance(self.scene_report, bool):
            raise ValueError(f"TEST.SCENE_REPORT must be true or false, got {self.scene_report!r}")
        self.scene_capsule_quantile = cfg.TEST.get("SCENE_CAPSULE_QUANTILE", 0.5)
        if isinstance(self.scene_capsule_quantile, bool) or not isinstance(self.scene_capsule_quantile, (int, float)) \
                or not 0 <= self.scene_capsule_quantile <= 1:
            raise ValueError(f"TEST.SCENE_CAPSULE_QUANTILE must be a number in 0..1, got {self.scene_capsule_quantile!r}")
        # estimate.py --track (seeme_amd/track.py): the random walk's step (mm per frame), the weight of the flow's density against the
        # transitions and the Gaussian width of the filter (frames).  None of the three was tuned on data.
        self.track_step_mm = check_step_mm(cfg.TEST.get("TRACK_STEP_MM", DEFAULT_STEP_MM), "TEST.TRACK_STEP_MM")
        self.track_prior_weight = check_prior_weight(cfg.TEST.get("TRACK_PRIOR_WEIGHT", DEFAULT_PRIOR_WEIGHT), "TEST.TRACK_PRIOR_WEIGHT")
        self.track_sigma = check_sigma(cfg.TEST.get("TRACK_SIGMA", DEFAULT_SIGMA), "TEST.TRACK_SIGMA")
        # PA-MPJPE, V2V and body-scene contact per hypothesis (seeme_amd/mesh_metrics.py): off = today's result, key for key
        self.mesh_metrics = cfg.TEST.get("MESH_METRICS", False)
        if not isinstance(self.mesh_metrics, bool):
            raise ValueError(f"TEST.MESH_METRICS must be true or false, got {self.mesh_metrics!r}")
        self.mesh_chunk_mb = cfg.TEST.get("MESH_CHUNK_MB", 256)
        if isinstance(self.mesh_chunk_mb, bool) or not isinstance(self.mesh_chunk_mb, (int, float)) or not self.mesh_chunk_mb > 0:
            raise ValueError(f"TEST.MESH_CHUNK_MB must be a positive number of MiB, got {self.mesh_chunk_mb!r}")
        # body-scene collision ratio per hypothesis (point-in-mesh test, seeme_amd/mesh_metrics.py); independent of TEST.MESH_METRICS
        self.collision_metrics = cfg.TEST.get("COLLISION_METRICS", False)
        if not isinstance(self.collision_metrics, bool):
            raise ValueError(f"TEST.COLLISION_METRICS must be true or false, got {self.collision_metrics!r}")
        if self.collision_metrics and "scene" not in self.condition:
            raise ValueError("TEST.COLLISION_METRICS needs the scene cloud, and model.condition has no 'scene': it would report nothing")
        # the evaluation by interpersonal distance and mutual gaze (seeme_amd/social_metrics.py): off = today's result, key for key
        self.social_metrics = cfg.TEST.get("SOCIAL_METRICS", False)
        if not isinstance(self.social_metrics, bool):
            raise ValueError(f"TEST.SOCIAL_METRICS must be true or false, got {self.social_metrics!r}")
        self.social_dist_edges = check_edges(cfg.TEST.get("SOCIAL_DIST_EDGES", list(DEFAULT_DIST_EDGES)), "TEST.SOCIAL_DIST_EDGES")
        self.social_gaze_edges = check_edges(cfg.TEST.get("SOCIAL_GAZE_EDGES", list(DEFAULT_GAZE_EDGES)), "TEST.SOCIAL_GAZE_EDGES",
                                             0.0, 180.0)
        if self.social_metrics:
            if self.data_type != "angle":
                raise ValueError(f"TEST.SOCIAL_METRICS needs DATA_TYPE 'angle' (got {self.data_type!r}): there are no orientation "
                                 "quaternions otherwise")
            if not self.predict_transl:
                raise ValueError("TEST.SOCIAL_METRICS needs TRAIN.ABLATION.PREDICT_TRANSL: without the translation in the features the "
                                 "two bodies are not in one frame")
            if self.estimate != "wearer":
                raise ValueError(f"TEST.SOCIAL_METRICS needs ESTIMATE 'wearer' (got {self.estimate!r}): the distances and angles are the "
                                 "wearer's to the interactee")
        # training-loop options (seeme_amd/optim.py): EMA of the trainable weights and clipping of the global gradient norm; 0 = off
        from .optim import check_options
        self.ema_decay, self.grad_clip_norm = check_options(cfg.TRAIN.get("EMA_DECAY", 0.0), cfg.TRAIN.get("GRAD_CLIP_NORM", 0.0),
                                                            names=("TRAIN.EMA_DECAY", "TRAIN.GRAD_CLIP_NORM"))
        self.ema_warmup = cfg.TRAIN.get("EMA_WARMUP", True)
        if not isinstance(self.ema_warmup, bool):
            raise ValueError(f"TRAIN.EMA_WARMUP must be true or false, got {self.ema_warmup!r}")
        self._ema_raw = None           # the raw weights while an ema_scope() is open
        self.hip_backward = cfg.TRAIN.get("HIP_BACKWARD", True)   # hand-written backward of the denoiser chain (one head)
        self.hip_vae_backward = cfg.TRAIN.get("HIP_VAE_BACKWARD", True)   # stage 1: hand-written VAE backward (vae_train.py)
        self.hip_glue = cfg.TRAIN.get("HIP_GLUE", True)           # ... and of everything around it (stage2_glue.py); needs HIP_BACKWARD
        self.pose_estimation_task = cfg.TEST.get("POSE_ESTIMATION_TASK", False)      # mld.py:116
        # mld.py:122-125; rot6d: 24 x 6 features, the translation outside them whatever PREDICT_TRANSL says, EgoBody only
        self.nfeats, self.transl_in_feats = motion_layout(self.name_dataset, self.data_type, self.predict_transl, cfg.model.nfeats)
        if "image" in self.condition and self.pose_estimation_task:
            raise NotImplementedError("TEST.POSE_ESTIMATION_TASK with an 'image' condition: the reference's dataset returns no interactee "
                                      "ground truth in the image batch layouts (dataset.py:1788-1792)")

        # SMPL (mld.py:151-153); frozen
        if smpl_model is not None:
            self.smpl_model = smpl_model
        else:
            self.smpl_model = SMPL(model_path=cfg.model.smpl_path, batch_size=cfg.TRAIN.BATCH_SIZE, gender="neutral")
        for p in self.smpl_model.parameters():
            p.requires_grad = False
        if self.collision_metrics:
            try:
                check_closed_faces(self.smpl_model.faces_tensor, int(self.smpl_model.v_template.shape[0]))
            except ValueError as e:
                raise ValueError(f"TEST.COLLISION_METRICS: smpl_model.faces_tensor is not a closed mesh: {e}") from e

        self.vae_type = cfg.model.get("vae_type", None) or \
            cfg.model.motion_vae.target.split(".")[-1].lower().replace("vae", "")      # mld.py:174-179
        # model.image_backbone: the frozen ResNet-50 (proscene.backbone) runs here and the image slot may hold crops; without it
        # batches carry its pooled [B,2048] features
        self.image_backbone = bool(cfg.model.get("image_backbone", False)) and "image" in self.condition
        if "image" in self.condition:                                     # mld.py:251-255; trainable in stage 2
            self.output_images = nn.Sequential(nn.ReLU(), nn.Linear(IMAGE_FEAT_DIM, 256))
        # model.interactee_head: ProHMR-scene's pose head (proscene.flow, seeme_amd/prohmr_head.py) for estimate_interactee; frozen,
        # always eval.  Off: no such entries in the state dict
        self.interactee_head = cfg.model.get("interactee_head", False)
        if not isinstance(self.interactee_head, bool):
            raise ValueError(f"model.interactee_head must be true or false, got {self.interactee_head!r}")
        # diag(axes) takes the recording's camera frame to the image's OpenCV frame, in which the head works (recording.opencv_views)
        from .recording import check_camera_axes
        self.interactee_camera_axes = check_camera_axes(cfg.TEST.get("INTERACTEE_CAMERA_AXES", [1, -1, -1]))
        if "scene" in self.condition or self.image_backbone or self.interactee_head:     # mld.py:182-207, 257-261
            self.proscene = _SceneEncoderHolder(scene="scene" in self.condition, backbone=self.image_backbone, flow=self.interactee_head)
            for p in self.proscene.parameters():
                p.requires_grad = False
        if self.image_backbone:
            # frozen, always eval; TRAIN.IMAGE_PRECISION bf16 runs bf16 weights and activations
            self.proscene.backbone.precision = cfg.TRAIN.get("IMAGE_PRECISION", self.proscene.backbone.precision)
        if "scene" in self.condition:
            # frozen scene encoder: TRAIN.SCENE_PRECISION bf16 runs the fused bf16-MFMA PointNet blocks
            self.proscene.scene_enc.precision = cfg.TRAIN.get("SCENE_PRECISION", self.proscene.scene_enc.precision)
            self.output_scene = nn.Sequential(nn.ReLU(), nn.Linear(512, 256))
        self.vae = instantiate_from_config(cfg.model.motion_vae)          # :264
        if self.stage == "diffusion":                                     # :267-271
            for p in self.vae.parameters():
                p.requires_grad = False
            # the frozen VAE only produces latents here: TRAIN.FROZEN_VAE_PRECISION fp16 runs it on the fp16-MFMA path
            self.vae.precision = cfg.TRAIN.get("FROZEN_VAE_PRECISION", self.vae.precision)
        self.denoiser = instantiate_from_config(cfg.model.denoiser)       # :282
        if not self.predict_epsilon:
            cfg.model.scheduler.params["prediction_type"] = "sample"
            cfg.model.noise_scheduler.params["prediction_type"] = "sample"
        self.scheduler = instantiate_from_config(cfg.model.scheduler)     # :286-287
        self.noise_scheduler = instantiate_from_config(cfg.model.noise_scheduler)
        if cfg.TRAIN.OPTIM.TYPE.lower() != "adamw":
            raise NotImplementedError("Do not support other optimizer for now.")
        self.optimizer = None          # built lazily: parameters must be on the device first
        self.losses = {k: MLDLosses(cfg) for k in ("train", "val", "test")}
        self.EgoMetric = EgoMetrics()
        self.HypMetric = HypothesisMetrics()
        self.MeshMetric = MeshMetrics()
        self.CollMetric = CollisionMetrics()
        self.SelMetric = SelectionMetrics()
        self.SocialMetric = SocialMetrics(self.social_dist_edges, self.social_gaze_edges)
        self.do_classifier_free_guidance = self.guidance_scale > 1.0
        self.renorm = datamodule.renorm if datamodule is not None else (lambda x: x)
        self.times: List[float] = []

    # ------------------------------------------------------------------ optimiser (mld.py:292-299, base.py:157-158)
    def configure_optimizers(self, capturable: bool = False):
        if self.optimizer is not None and capturable and not self.optimizer.param_groups[0].get("capturable", False):
            raise RuntimeError("configure_optimizers(capturable=True): an optimiser built with capturable=False exists "
                               "(capture_training_step does not need a capturable torch AdamW: it uses seeme_adamw_step_dev)")
        if self.optimizer is None:
            params = [p for p in self.parameters() if p.requires_grad]
            self.optimizer = torch.optim.AdamW(params, lr=self.cfg.TRAIN.OPTIM.LR, capturable=capturable)
            self.sch = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=self.cfg.TRAIN.OPTIM.STEP_SIZE,
                                                       gamma=self.cfg.TRAIN.OPTIM.GAMMA)
            # eager steps update all tensors in one launch (seeme_adamw_step) on this optimiser's own state; the
            # hipGraph-captured step (capturable=True) stays on PyTorch's AdamW
            self._fused_adamw = self._torch_adamw = None
            opts = dict(ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, grad_clip_norm=self.grad_clip_norm)
            if not capturable and bool(self.cfg.TRAIN.get("FUSED_ADAMW", True)) and params and all(p.is_cuda for p in params):
                from .optim import FusedAdamWStep
                self._fused_adamw = FusedAdamWStep(self.optimizer, **opts)
            elif self.ema_decay > 0.0 or self.grad_clip_norm > 0.0:
                from .optim import TorchAdamWStep
                self._torch_adamw = TorchAdamWStep(self.optimizer, **opts)      # the same three steps in PyTorch operations
        return {"optimizer": self.optimizer}

    def _stepper(self):
        return getattr(self, "_fused_adamw", None) or getattr(self, "_torch_adamw", None)

    def optimizer_update(self):
        """The AdamW update of the trainable tensors (after backward and the gradient all-reduce), with TRAIN.GRAD_CLIP_NORM and
        TRAIN.EMA_DECAY when they are on."""
        if self._ema_raw is not None:
            raise RuntimeError("optimizer step inside ema_scope(): the parameters hold the EMA weights")
        st = self._stepper()
        if st is not None:
            st.step()
        else:
            self.optimizer.step()

    @property
    def last_grad_norm(self):
        """{norm, scale} of the last clipped step as a device tensor (None before it, or with TRAIN.GRAD_CLIP_NORM 0): reading a
        value synchronises, so the training loop reads it at the epoch's end."""
        st = self._stepper()
        return st.last_grad_norm if st is not None else None

    # ------------------------------------------------------------------ EMA weights (TRAIN.EMA_DECAY)
    def _ema_pairs(self):
        """(name in state_dict(), parameter, shadow) of every trainable tensor."""
        st = self._stepper()
        if st is None or self.ema_decay <= 0.0:
            raise RuntimeError("EMA is off (TRAIN.EMA_DECAY 0, or configure_optimizers() has not run)")
        st._ensure_shadows()
        return [(n, p, st.shadow[p]) for n, p in self.named_parameters() if p in st.shadow]

    def ema_state_dict(self):
        return {n: e for n, _, e in self._ema_pairs()}

    @torch.no_grad()
    def load_ema_state_dict(self, sd, strict: bool = True):
        pairs = self._ema_pairs()
        if strict:
            missing, unexpected = [n for n, _, _ in pairs if n not in sd], sorted(set(sd) - {n for n, _, _ in pairs})
            if missing or unexpected:
                raise RuntimeError(f"load_ema_state_dict: missing {missing}, unexpected {unexpected}")
        for n, _, e in pairs:
            if n in sd:
                if tuple(sd[n].shape) != tuple(e.shape):
                    raise RuntimeError(f"load_ema_state_dict: {n} has shape {tuple(sd[n].shape)}, expected {tuple(e.shape)}")
                e.copy_(sd[n])

    @contextlib.contextmanager
    def ema_scope(self):
        """The EMA weights in the parameters for the length of the block, the raw weights back on exit (also on an exception).  The
        copies are in place -- captured graphs and pointer tables keep the parameters' addresses -- and bump the version counters,
        so the sampling-side weight images rebuild on entry and on exit.  Not re-entrant; no optimiser step inside."""
        pairs = self._ema_pairs()
        if self._ema_raw is not None:
            raise RuntimeError("ema_scope() is not re-entrant")
        with torch.no_grad():
            self._ema_raw = [p.detach().clone() for _, p, _ in pairs]
            try:
                for _, p, e in pairs:
                    p.copy_(e)
                yield self
            finally:
                for (_, p, _), raw in zip(pairs, self._ema_raw):
                    p.copy_(raw)
                self._ema_raw = None

    def trainable_parameters(self):
        return [p for p in self.parameters() if p.requires_grad]

    # ------------------------------------------------------------------ condition assembly
    def _scene_token(self, scene, cfg_mask_train=False, mask=None, code_only=False):
        scene = scene.float()
        if cfg_mask_train and self.do_classifier_free_guidance:           # mld.py:917-919
            if mask is None:
                mask = torch.rand_like(scene) < self.guidance_uncodp
            scene = scene.masked_fill(mask, 0.0)
        s512 = self.proscene.encode_scene(scene)                          # HIP PointNet
        if code_only:
            return s512
        # output_scene = ReLU + Linear(512,256) (trainable, mld.py:257-261): torch op so that autograd sees it
        return self.output_scene(s512).unsqueeze(0)                       # [1,B,256]

    def _image_feats(self, images) -> torch.Tensor:
        """The image slot of a batch -> pooled backbone features [B,2048] (what proscene.encode_image returns, mld.py:895-896):
        features pass through; with model.image_backbone crops (float32 NCHW [B,3,224,224] normalised, or uint8 NHWC
        [B,224,224,3] RGB) run through the HIP ResNet-50, once per sequence."""
        if not torch.is_tensor(images):
            raise TypeError(f"the image slot of the batch holds {type(images).__name__}: expected pooled image features [B,{IMAGE_FEAT_DIM}]")
        if images.dim() == 4 and self.image_backbone:
            with torch.no_grad():
                return self.proscene.encode_image(images)
        if images.dim() == 4:
            raise NotImplementedError(f"the image slot holds images {tuple(images.shape)}: the ResNet-50 backbone (proscene.encode_image) "
                                      f"is off -- set model.image_backbone: true, or pass its pooled features [B,{IMAGE_FEAT_DIM}] (INTEGRATION.md)")
        if images.dim() != 2 or images.shape[1] != IMAGE_FEAT_DIM or not images.is_floating_point():
            raise ValueError(f"image features are {tuple(images.shape)} {images.dtype}: expected float [B,{IMAGE_FEAT_DIM}]")
        return images.float()

    def _image_token(self, images) -> torch.Tensor:
        # output_images = ReLU + Linear(2048,256) (trainable, mld.py:251-255): torch op, as output_scene above
        return self.output_images(self._image_feats(images)).unsqueeze(0)   # [1,B,256]

    def _wearer_features(self, feats_ref, transl, idx):
        f = feats_ref[:, :, idx, :]
        if self.transl_in_feats:
            f = torch.cat([f, transl[:, idx, :, :]], dim=-1)
        if f.shape[-1] != self.vae.nfeats:
            raise ValueError(f"motion features are {f.shape[-1]} wide (pose {feats_ref.shape[-1]}"
                             f"{' + 3 translation' if self.transl_in_feats else ''}) but the VAE was built with nfeats "
                             f"{self.vae.nfeats} (model.nfeats)")
        return f.contiguous()

    def _sample_latent(self, feats, lengths, eps=None, mean=False):
        """vae.encode(...)[0] of the reference (a posterior sample, mld_vae.py:186-193) with the noise injectable:
        eps [1,B,256] replaces the draw; mean=True returns mu.  Returns (z [1,B,256], Normal)."""
        dist = self.vae.encode_dist(feats, lengths)
        mu, std = dist[0:1], dist[1:2].exp().pow(0.5)
        normal = torch.distributions.Normal(mu, std, validate_args=False)
        if mean:
            return mu, normal
        if eps is None:
            eps = torch.empty_like(mu).normal_()
        return mu + eps.to(mu) * std, normal

    # ------------------------------------------------------------------ the sampling steps of ego_eval and predict
    @staticmethod
    def _rep_rows(t, K: int):
        """[1,B,256] -> [1,B*K,256], row b*K + k = row b; K = 1 is `t` itself (no launch)."""
        return t if K == 1 else t.repeat_interleave(K, dim=1)

    def _condition_tokens(self, scene, images, K: int, who: str):
        """(scene_tok, img_tok) of a sampling pass, each [1,B*K,256] or None; scene_tok is [1,2*B*K,256] under guidance.  The encoders
        run once per sequence, on B rows, and the tokens are repeated K times.  Stage 'vae' conditions on nothing.  `who` names the
        caller in the error message."""
        scene_tok = img_tok = None
        if self.stage == "vae":
            return scene_tok, img_tok
        if images is not None:
            if self.do_classifier_free_guidance:
                raise NotImplementedError(f"{who} with an 'image' condition and guidance_scale > 1: the reference builds no unconditional "
                                          "scene / image token in the image branches of ego_eval (mld.py:1076-1100) while _diffusion_reverse "
                                          "halves the batch (:437-438), so that configuration cannot run; training with it is defined (DESIGN 6a)")
            img_tok = self._rep_rows(self._image_token(images), K)         # (no unconditional image token: see above)
            if scene is not None:
                scene_tok = self._rep_rows(self._scene_token(scene), K)
        elif scene is not None:
            scene_tok = self._rep_rows(self._scene_token(scene), K)
            if self.do_classifier_free_guidance:                           # zero-scene branch (:1144-1158)
                unc = self._rep_rows(self._scene_token(torch.zeros_like(scene)), K)
                # the reference concatenates [scene, scene_uncond] while _diffusion_reverse takes the FIRST half as
                # unconditional (:489): reproduced by default, TEST.CFG_SCENE_ORDER 'fixed' puts uncond first
                scene_tok = torch.cat([scene_tok, unc] if self.cfg_scene_order == "reference" else [unc, scene_tok], dim=1)
        return scene_tok, img_tok

    def _posterior_draws(self, feats, lengths, eps, K: int):
        """K posterior draws per sequence from ONE encode: [1,B*K,256], the posterior mean under TEST.SAMPLE_MEAN.  eps [1,B*K,256]
        replaces the draw.  For K = 1 this is _sample_latent without the Normal object."""
        dist = self.vae.encode_dist(feats, lengths)
        mu, std = self._rep_rows(dist[0:1], K), self._rep_rows(dist[1:2].exp().pow(0.5), K)
        if self.sample_mean:
            return mu
        if eps is None:
            eps = torch.empty_like(mu).normal_()
        return mu + eps.to(mu).reshape(mu.shape) * std

    def _condition_rows(self, f_int, lengths, eps_c, eps_u, scene_tok, img_tok, K: int):
        """The denoiser's condition, batch-first [B*K or 2*B*K, N, 256] (unconditional rows first with guidance): the tokens
        [text, scene, images] (:1297-1306), text = K draws of the interactee's posterior (f_int None: no such token; :1271-1295)."""
        text_emb = None
        if f_int is not None:
            text_emb = self._posterior_draws(f_int, lengths, eps_c, K)
            if self.do_classifier_free_guidance:
                text_emb = torch.cat([self._posterior_draws(torch.zeros_like(f_int), lengths, eps_u, K), text_emb], dim=1)
        toks = [t for t in (text_emb, scene_tok, img_tok) if t is not None]
        if not toks:
            raise ValueError("no condition tokens")
        return torch.cat(toks, dim=0).permute(1, 0, 2)

    # ------------------------------------------------------------------ reverse diffusion (mld.py:432-511)
    def _reverse_setup(self, latents):
        """The initial latents scaled for the scheduler, whose inference timesteps are set here, and the eta of its step."""
        latents = latents * self.scheduler.init_noise_sigma
        self.scheduler.set_timesteps(self.cfg.model.scheduler.num_inference_timesteps)
        eta = 0.0
        if "eta" in set(inspect.signature(self.scheduler.step).parameters.keys()):
            eta = self.cfg.model.scheduler.eta
        return latents, eta

    def _diffusion_reverse(self, encoder_hidden_states, lengths=None, latents=None, step_noise=None):
        bsz = encoder_hidden_states.shape[0]
        if self.do_classifier_free_guidance:
            bsz = bsz // 2
        if latents is None:
            latents = torch.randn((bsz, self.latent_dim[0], self.latent_dim[-1]), device=encoder_hidden_states.device,
                                  dtype=torch.float)
        latents, eta = self._reverse_setup(latents)
        # the 50 (or 1000) sequential denoiser calls + CFG + scheduler.step are ONE kernel launch
        return self.denoiser.sample_loop(latents, encoder_hidden_states.contiguous(), self.scheduler, eta=eta,
                                         guidance_scale=self.guidance_scale if self.do_classifier_free_guidance else 1.0,
                                         step_noise=step_noise)            # [1,B,256]

    # ------------------------------------------------------------------ forward diffusion (mld.py:582-631)
    def _diffusion_process(self, latents, encoder_hidden_states, lengths=None, noise=None, timesteps=None):
        latents = latents.permute(1, 0, 2)
        if noise is None:
            noise = torch.randn_like(latents)
        bsz = latents.shape[0]
        if timesteps is None:
            timesteps = torch.randint(0, self.noise_scheduler.config.num_train_timesteps, (bsz,), device=latents.device)
        timesteps = timesteps.long()
        noisy = self.noise_scheduler.add_noise(latents.clone(), noise, timesteps)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.denoiser.parameters()):
            from .denoiser_train import denoiser_forward_hip_train, hip_train_supported
            if self.hip_backward and noisy.is_cuda and hip_train_supported(self.denoiser, encoder_hidden_states.shape[0]):
                noise_pred = denoiser_forward_hip_train(self.denoiser, noisy, timesteps, encoder_hidden_states)  # HIP fwd + bwd
            else:
                if self.hip_backward and noisy.is_cuda:
                    _warn_once("denoiser", "stage-2 training of this denoiser configuration (more than one attention head, or a shape the "
                               "hand-written backward does not cover) runs on the PyTorch-autograd twin (seeme_amd/denoiser_autograd.py): correct, "
                               "several times slower than the HIP forward/backward")
                noise_pred = denoiser_forward_torch(self.denoiser, noisy, timesteps, encoder_hidden_states)  # autograd twin
        else:
            noise_pred = self.denoiser(sample=noisy, timestep=timesteps, encoder_hidden_states=encoder_hidden_states,
                                       lengths=lengths)[0]                                              # HIP
        n_set = {"noise": noise, "noise_prior": 0, "noise_pred": noise_pred, "noise_pred_prior": 0}
        if not self.predict_epsilon:
            n_set["pred"] = noise_pred
            n_set["latent"] = latents
        return n_set

    # ------------------------------------------------------------------ stage-2 training forward (mld.py:887-1017)
    def train_diffusion_forward(self, batch, noise=None, timesteps=None, eps=None, masks=None):
        """Injection points for parity tests (not in the reference), in the order the reference draws: masks =
        (scene mask, interactee mask) -- the boolean results of ``rand_like(x) < guidance_uncondp`` (:917-919, :966-968),
        eps = (target rsample noise, condition rsample noise) [1,B,256] each, then `noise` and `timesteps` (:591-601)."""
        m_scene, m_int = masks if masks is not None else (None, None)
        e_z, e_c = eps if eps is not None else (None, None)
        feats_ref, transl, beta, utils_, scene, images, length, _ = split_batch(self.condition, batch)
        if images is not None:
            images = self._image_feats(images)                                # [B,2048] (no input mask: mld.py:889-909)
        if scene is not None:
            # the classifier-free input mask of the scene exists only without an image (mld.py:889-922)
            scene = self._scene_token(scene, cfg_mask_train=images is None, mask=m_scene, code_only=True)      # [B,512] PointNet code
        feats_ref, transl = feats_ref.float(), transl.float()
        lengths = [feats_ref.shape[1]] * feats_ref.shape[0]
        n_tok = int(scene is not None) + int(images is not None) + int("interactee" in self.condition)
        glue = self._stage2_glue(n_tok) if feats_ref.is_cuda else None
        if glue is not None:
            return self._train_diffusion_forward_glue(glue, feats_ref, transl, scene, lengths, noise, timesteps, e_z, e_c, m_int, images)
        if scene is not None:
            scene = self.output_scene(scene).unsqueeze(0)                     # [1,B,256]
        if images is not None:
            images = self.output_images(images).unsqueeze(0)                  # [1,B,256]
        with torch.no_grad():
            idx = 0 if self.estimate == "wearer" else 1
            f_tgt = self._wearer_features(feats_ref, transl, idx)
            z_cond = None
            B = f_tgt.shape[0]
            shape = (1, B, self.vae.latent_dim)
            draw = lambda e: torch.empty(shape, device=f_tgt.device, dtype=torch.float32).normal_() if e is None else e.to(f_tgt)
            if "interactee" in self.condition:
                # target and interactee go through the frozen VAE as ONE batch of 2B sequences (the encode is a chain of
                # ~20 latency-bound launches); the three random draws keep the order of the two separate encodes:
                # rsample noise of the target, the CFG input mask, rsample noise of the condition (mld.py:944-984)
                eps_z = draw(e_z)
                f_int = self._wearer_features(feats_ref, transl, 1)
                if self.do_classifier_free_guidance:                       # mld.py:966-981
                    mask = (torch.rand_like(f_int) < self.guidance_uncodp) if m_int is None else m_int
                    f_int = f_int.masked_fill(mask, 0.0)
                eps_c = draw(e_c)
                dist = self.vae.encode_dist(torch.cat([f_tgt, f_int], dim=0), lengths + lengths)      # [2, 2B, 256]
                mu, std = dist[0:1], dist[1:2].exp().pow(0.5)              # mld_vae.py:186-190
                z = mu[:, :B] + eps_z * std[:, :B]                         # Normal(mu, std).rsample(), :192
                z_cond = mu[:, B:] + eps_c * std[:, B:]
            else:
                z, _ = self._sample_latent(f_tgt, lengths, e_z)
        toks = [t for t in (z_cond, scene, images) if t is not None]      # :991-1013: [z_cond, scene, images] in this order
        if not toks:
            raise ValueError("no condition: MldDenoiser needs at least one condition token")
        cond_emb = torch.cat(toks, dim=0) if len(toks) > 1 else toks[0]
        return {**self._diffusion_process(z, cond_emb, lengths, noise=noise, timesteps=timesteps)}

    def _vae_trainer(self, T: int):
        """The hand-written stage-1 forward / backward (vae_train.VaeTrainer) when this model can take it."""
        if not self.hip_vae_backward:
            return None
        from .vae_train import VaeTrainer
        if not VaeTrainer.supported(self.vae, T):
            _warn_once("vae", "stage-1 training of this VAE configuration (more than one attention head, or more than 512 tokens) runs on the "
                       "PyTorch-autograd twin (seeme_amd/vae_autograd.py): correct, several times slower than the HIP forward/backward")
            return None
        t = getattr(self, "_vae_tr", None)
        if t is None or t.stale():
            t = VaeTrainer(self.vae)
            object.__setattr__(self, "_vae_tr", t)
        return t

    def _stage2_glue(self, n_tokens: int):
        """The hand-written forward/backward around the chain (stage2_glue.Stage2Glue) when this step can take it."""
        if not (self.hip_glue and self.hip_backward and torch.is_grad_enabled() and n_tokens >= 1):
            return None
        from .stage2_glue import Stage2Glue
        if not any(p.requires_grad for p in self.denoiser.parameters()) or not Stage2Glue.supported(self, n_tokens):
            return None
        g = getattr(self, "_glue", None)
        if g is None or g.stale():
            g = Stage2Glue(self)
            object.__setattr__(self, "_glue", g)
        return g

    def _train_diffusion_forward_glue(self, glue, feats_ref, transl, s512, lengths, noise, timesteps, e_z, e_c, m_int, img=None):
        """train_diffusion_forward + _diffusion_process with everything between the frozen encoders and the loss in
        stage2_glue's kernels; the random draws keep the reference's order (mld.py:917-919,944-984,591-601)."""
        with torch.no_grad():
            idx = 0 if self.estimate == "wearer" else 1
            f_tgt = self._wearer_features(feats_ref, transl, idx)
            B, dev = f_tgt.shape[0], f_tgt.device
            draw = lambda e: torch.empty(B, 256, device=dev, dtype=torch.float32).normal_() if e is None else e.to(f_tgt).reshape(B, 256)
            eps_z = draw(e_z)
            eps_c = None
            if "interactee" in self.condition:
                f_int = self._wearer_features(feats_ref, transl, 1)
                if self.do_classifier_free_guidance:                       # mld.py:966-981
                    mask = (torch.rand_like(f_int) < self.guidance_uncodp) if m_int is None else m_int
                    f_int = f_int.masked_fill(mask, 0.0)
                eps_c = draw(e_c)
                dist = self.vae.encode_dist(torch.cat([f_tgt, f_int], dim=0), lengths + lengths)      # [2, 2B, 256]
            else:
                dist = self.vae.encode_dist(f_tgt, lengths)
            noise = torch.randn(B, 1, 256, device=dev) if noise is None else noise.to(f_tgt)
            if timesteps is None:
                timesteps = torch.randint(0, self.noise_scheduler.config.num_train_timesteps, (B,), device=dev)
        noise_pred, latents = glue(dist, eps_z, eps_c, noise, timesteps.long(), s512, img)
        n_set = {"noise": noise.reshape(B, 1, 256), "noise_prior": 0, "noise_pred": noise_pred, "noise_pred_prior": 0}
        if not self.predict_epsilon:
            n_set["pred"] = noise_pred
            n_set["latent"] = latents
        return n_set

    # ------------------------------------------------------------------ stage-1 forward (mld.py:633-885)
    def train_vae_forward(self, batch, eps=None):
        """encode -> rsample -> decode -> renorm -> SMPL joints of reference and reconstruction.  m_ref / m_rst are the
        RENORMED features, as in the reference (mld.py:757,778,871-878).  GIMO keeps the first 21 joints and poses the
        reconstruction with the reference's global orientation (:826-828,852-859).  eps [1,B,256]: injected rsample noise."""
        feats_ref, transl, beta = batch[0].float(), batch[1].float(), batch[2].float()
        lengths = [feats_ref.shape[1]] * feats_ref.shape[0]
        idx = 0 if self.estimate == "wearer" else 1
        f_ref = self._wearer_features(feats_ref, transl, idx)
        gimo = self.name_dataset == "gimo" and self.data_type == "angle"
        nj = 21 if gimo else 24
        m_ref = self.renorm(f_ref)
        ref_orient = m_ref[:, :, :3] if gimo else None
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.vae.parameters()):
            # stage-1 training: differentiable twins of the VAE and the SMPL joint regressor (PyTorch-ROCm autograd)
            tr = self._vae_trainer(f_ref.shape[1]) if f_ref.is_cuda else None
            if tr is not None:        # hand-written HIP forward-with-saves / backward of the encoder and the decoder (vae_train.py)
                mu, logvar = tr.encode(f_ref, lengths)
                std = logvar.exp().pow(0.5)
                dec = tr.decode
            else:                     # differentiable twins on PyTorch autograd
                from .vae_autograd import vae_encode_torch, vae_decode_torch
                mu, std = vae_encode_torch(self.vae, f_ref, lengths)
                dec = lambda zz, ll: vae_decode_torch(self.vae, zz, ll)
            dist_m = torch.distributions.Normal(mu, std, validate_args=False)
            z = dist_m.rsample() if eps is None else mu + eps.to(mu) * std
            m_rst = self.renorm(dec(z, lengths))                           # differentiable (geometry._Renorm)
            with torch.no_grad():
                if self.data_type == "rot6d" and m_ref.is_cuda:            # one fused launch (seeme_smpl_joints_rot6d)
                    joints_ref = self._rot6d_joints(m_ref, hip=True)
                else:
                    joints_ref = self._feats_to_joints(m_ref, beta[:, idx])[:, :, :nj]
            joints_rst = self._feats_to_joints_torch(m_rst, beta[:, idx], orient=ref_orient)[:, :, :nj]
        else:
            z, dist_m = self._sample_latent(f_ref, lengths, eps)
            m_rst = self.renorm(self.vae.decode(z, lengths))
            joints_ref = self._feats_to_joints(m_ref, beta[:, idx])[:, :, :nj]
            joints_rst = self._feats_to_joints(m_rst, beta[:, idx], orient=ref_orient)[:, :, :nj]
        if self.is_vae:                                                    # mld.py:683-691
            dist_ref = torch.distributions.Normal(torch.zeros_like(dist_m.loc), torch.ones_like(dist_m.scale))
        else:
            dist_ref = dist_m
        return {"m_ref": m_ref, "m_rst": m_rst, "joints_ref": joints_ref, "joints_rst": joints_rst,
                "dist_m": dist_m, "dist_ref": dist_ref, "lat_m": z.permute(1, 0, 2)}

    # ------------------------------------------------------------------ features -> SMPL joints
    def _feats_to_joints(self, feats, betas, want_vertices=False, orient=None):
        """feats [B,T,F] (renormed).  'angle': [global_orient 3 | body_pose 21..23 joints | transl 3];
        'rot6d': 24 x 6 (the reference builds that body model in float64, mld.py:161-163).  orient [B,T,3]: global
        orientation to pose with instead of the features' own.  Returns joints [B,T,24,3] (and vertices)."""
        B, T, F = feats.shape
        if self.data_type == "rot6d":                                      # mld.py:1410-1449
            R = G.rot6d_to_rotmat(feats[..., :144].reshape(-1, 6).contiguous()).reshape(B * T, 24, 3, 3)
            zb = torch.zeros(B * T, 10, device=feats.device, dtype=torch.float32)     # create_beta=False: betas are not passed
            out = self.smpl_model(betas=zb, body_pose=R[:, 1:], global_orient=R[:, 0:1],
                                  pose2rot=False, return_verts=want_vertices, transl=None)
        else:
            nb = 69 if self.name_dataset == "egobody" else 63
            body = feats[:, :, 3:3 + nb].reshape(-1, nb).float()
            if nb < 69:                                                    # GIMO pads 21 -> 23 joints (mld.py:807-813)
                body = torch.cat([body, torch.zeros(body.shape[0], 69 - nb, device=body.device)], dim=1)
            go = (feats[:, :, :3] if orient is None else orient).reshape(-1, 3).float()
            tr = feats[:, :, -3:].reshape(-1, 3).float().contiguous() if self.predict_transl else None
            out = self.smpl_model(betas=betas.reshape(-1, 10).float(), body_pose=body.contiguous(),
                                  global_orient=go.contiguous(), transl=tr, pose2rot=True, return_verts=want_vertices)
        joints = out.joints.reshape(B, T, 45, 3)[:, :, :24]                # mld.py:771-773
        if want_vertices:
            return joints, out.vertices.reshape(B, T, -1, 3)
        return joints

    def _feats_to_joints_torch(self, feats, betas, orient=None):
        """Differentiable version of _feats_to_joints for stage-1 training.  'rot6d' (mld.py:703-742): the first 144 features, zero
        betas, no translation, `orient` ignored."""
        from .vae_autograd import smpl_joints_torch
        if self.data_type == "rot6d":
            return self._rot6d_joints(feats, hip=self.hip_vae_backward and feats.is_cuda)
        B, T, _ = feats.shape
        nb = 69 if self.name_dataset == "egobody" else 63
        pose = feats[:, :, :3 + nb]
        if orient is not None:
            pose = torch.cat([orient.to(pose), pose[:, :, 3:]], dim=-1)
        pose = pose.reshape(B * T, 3 + nb)
        if nb < 69:                                                        # GIMO pads 21 -> 23 joints (mld.py:807-813)
            pose = torch.cat([pose, torch.zeros(B * T, 69 - nb, device=pose.device, dtype=pose.dtype)], dim=1)
        tr = feats[:, :, -3:].reshape(B * T, 3) if self.predict_transl else None
        if self.hip_vae_backward and pose.is_cuda:           # HIP forward + hand-written backward (smpl._JointsAA)
            from .smpl import smpl_joints_hip
            return smpl_joints_hip(self.smpl_model, betas.reshape(-1, 10).float(), pose.float(), tr).reshape(B, T, 24, 3)
        return smpl_joints_torch(self.smpl_model, betas.reshape(-1, 10).float(), pose.float(), tr).reshape(B, T, 24, 3)

    def _rot6d_joints(self, feats, hip: bool):
        """[B,T,24,3] joints of renormed rot6d features [B,T,>=144] (model-side element order, zero betas, no translation),
        differentiable: the fused HIP forward / hand-written backward (smpl._JointsRot6d) or the autograd twin."""
        B, T, _ = feats.shape
        r6 = feats[:, :, :144].reshape(B * T, 24, 6).float()
        if hip:
            from .smpl import smpl_joints_rot6d_hip
            return smpl_joints_rot6d_hip(self.smpl_model, None, r6, None).reshape(B, T, 24, 3)
        from .vae_autograd import smpl_joints_rot6d_torch
        return smpl_joints_rot6d_torch(self.smpl_model, None, r6, None).reshape(B, T, 24, 3)

    # ------------------------------------------------------------------ evaluation (mld.py:1076-1905, live part)
    @torch.no_grad()
    def ego_eval(self, batch, latents=None, want_vertices=False, cond_noise=None, step_noise=None, num_hypotheses=None,
                 hyp_select=None):
        """Injection points for parity tests (not in the reference): latents [B,1,256] initial noise; cond_noise = eps
        [1,B,256] of the condition sample (stage 'vae': of the target's sample), or a pair (eps_cond, eps_uncond) with
        classifier-free guidance; step_noise for DDPM.

        num_hypotheses K (None: TEST.NUM_HYPOTHESES) > 1 draws K hypotheses per sequence from ONE encode of the condition
        (``_ego_eval_hypotheses``): the injection points then have B*K rows, row b*K + k = hypothesis k of sequence b.  Both paths (and
        ``predict``) build the condition with the same steps (``_condition_tokens``, ``_posterior_draws``, ``_condition_rows``); K = 1's
        own, below, are the single sampling launch for any B (``_diffusion_reverse``) and the single decode.  hyp_select (None:
        TEST.HYP_SELECT) 'first' | 'medoid' chooses the hypothesis that fills the keys of a K = 1 result; it applies only for K > 1."""
        K = self.num_hypotheses if num_hypotheses is None else self._check_num_hypotheses(num_hypotheses, "num_hypotheses")
        select = self.hyp_select if hyp_select is None else check_select(hyp_select, "hyp_select")
        int_gt = None
        if self.pose_estimation_task:       # batch ends with the interactee's ground truth (mld.py:1119-1131)
            batch, int_gt = tuple(batch[:-3]), tuple(t.float() for t in batch[-3:])
        if K > 1:
            return self._ego_eval_hypotheses(batch, int_gt, K, latents, want_vertices, cond_noise, step_noise, select)
        eps_c, eps_u = cond_noise if isinstance(cond_noise, (tuple, list)) else (cond_noise, None)
        # image layouts: `length` last, as the dataset hands it over (the reference's unpack at :1079 / :1093 omits it: DESIGN 6a)
        feats_ref, transl, beta, utils_, scene, images, length, _ = split_batch(self.condition, batch)
        scene_tok, img_tok = self._condition_tokens(scene, images, 1, "ego_eval")
        feats_ref, transl, beta = feats_ref.float(), transl.float(), beta.float()
        lengths = length.long().reshape(-1).tolist()
        idx_ref = 0 if self.estimate == "wearer" else 1
        start = time.time()
        if self.stage in ("diffusion", "vae_diffusion"):
            f_int = self._wearer_features(feats_ref, transl, 1) if "interactee" in self.condition else None
            cond_bf = self._condition_rows(f_int, lengths, eps_c, eps_u, scene_tok, img_tok, 1)      # [B or 2B, N, 256]
            z = self._diffusion_reverse(cond_bf, lengths, latents=latents, step_noise=step_noise)
        elif self.stage == "vae":                                          # :1328-1352: reconstruction of the target itself
            z = self._posterior_draws(self._wearer_features(feats_ref, transl, idx_ref), lengths, eps_c, 1)
        else:
            raise ValueError(f"Not support this stage {self.stage}!")
        if self.see_future:
            lengths = [int(i // 2) for i in lengths]
        feats_rst = self.vae.decode(z, lengths)
        self.times.append(time.time() - start)                              # mld.py:1367-1368
        min_len = min(feats_ref.shape[1], feats_rst.shape[1])
        f_ref = self._wearer_features(feats_ref[:, :min_len], transl[:, :, :min_len], idx_ref)
        f_ref, f_rst = self.renorm(f_ref), self.renorm(feats_rst[:, :min_len].contiguous())
        b_ref = beta[:, idx_ref, :min_len]
        # egobody: TEST.GLOBAL_ORIENT_PRED False poses the prediction with the reference orientation (:1497-1501)
        o_rst = f_ref[:, :, :3] if (self.data_type == "angle" and self.name_dataset == "egobody" and not self.pred_global_orient) else None
        out_ref = self._feats_to_joints(f_ref, b_ref, want_vertices)
        out_rst = self._feats_to_joints(f_rst, b_ref, want_vertices, orient=o_rst)
        joints_ref, joints_rst = (out_ref[0], out_rst[0]) if want_vertices else (out_ref, out_rst)
        f_int_r = self.renorm(self._wearer_features(feats_ref[:, :min_len], transl[:, :, :min_len], 1))
        joints_int = self._feats_to_joints(f_int_r, beta[:, 1, :min_len])
        joints_int_gt = self._interactee_gt_joints(int_gt, beta, min_len)
        rs = {"m_ref": f_ref, "m_rst": f_rst, "joints_ref": joints_ref, "joints_rst": joints_rst,
              "orientation_quat_rst": self._orientation_quat(f_rst, o_rst), "orientation_quat_ref": self._orientation_quat(f_ref),
              "root_interactee": joints_int[:, :, 0], "joints_interactee": joints_int,
              "orientation_quat_int": self._orientation_quat(f_int_r), "joints_interactee_gt": joints_int_gt, "lengths": lengths,
              "list_names": {}, "lat_t": z}
        if want_vertices:
            rs["vertices_ref"], rs["vertices_rst"] = out_ref[1], out_rst[1]
        self._add_mesh_results(rs, f_rst, f_ref, b_ref, o_rst, lengths, 1, scene)
        if self.social_metrics:
            rs["social_metrics"] = social_metrics_hip(joints_rst[:, None], joints_ref, joints_int, rs["orientation_quat_rst"],
                                                      rs["orientation_quat_ref"], rs["orientation_quat_int"], lengths)
        return rs

    def _interactee_gt_joints(self, int_gt, beta, min_len):
        """SMPL joints of the interactee's ground-truth motion (TEST.POSE_ESTIMATION_TASK, mld.py:1843-1866); None without it."""
        if int_gt is None:
            return None
        g_motion, g_transl, _g_beta = int_gt
        f_gt = g_motion[:, :min_len, 0]
        if self.transl_in_feats:
            f_gt = torch.cat([f_gt, g_transl[:, 0, :min_len]], dim=-1)
        return self._feats_to_joints(self.renorm(f_gt.contiguous()), beta[:, 1, :min_len])

    def _orientation_quat(self, f, o=None):
        """[rows*T,4] quaternions of the global orientation of renormed 'angle' features [rows,T,F], or of `o` [rows,T,3] in its
        place; None for other data types."""
        if self.data_type != "angle":
            return None
        return G.aa_to_quat((f[:, :, :3] if o is None else o).reshape(-1, 3).contiguous())

    def _mesh_metrics(self, f_rst, f_ref, b_ref, orient, lengths, K, scene, mesh=True, collision=False):
        """TEST.MESH_METRICS: PA_MPJPE, V2V [B,K] and, with a scene in the batch, SCENE_DIST, CONTACT_RATIO [B,K] and their _REF
        forms [B] (seeme_amd.mesh_metrics.mesh_metrics_eval: posed and measured in chunks of TEST.MESH_CHUNK_MB MiB of vertices).
        collision: COLLISION_RATIO, COLLISION_FRAMES [B,K] and their _REF forms [B] as well, from the same posed chunks; mesh False
        leaves the first group out."""
        pose = lambda feats, betas, o: self._feats_to_joints(feats, betas, True, orient=o)
        if collision and scene is None:
            raise ValueError("TEST.COLLISION_METRICS: the batch carries no scene cloud")
        return mesh_metrics_eval(pose, f_rst, f_ref, b_ref, orient, lengths, K, scene=scene, chunk_mb=self.mesh_chunk_mb,
                                 num_vertices=int(self.smpl_model.v_template.shape[0]),
                                 faces=self.smpl_model.faces_tensor if collision else None, mesh=mesh)

    def _collision_metrics(self, f_rst, f_ref, b_ref, orient, lengths, K, scene):
        """TEST.COLLISION_METRICS alone: the four collision keys."""
        return self._mesh_metrics(f_rst, f_ref, b_ref, orient, lengths, K, scene, mesh=False, collision=True)

    def _add_mesh_results(self, rs, f_rst, f_ref, b_ref, orient, lengths, K, scene):
        """rs['mesh_metrics'] under TEST.MESH_METRICS, rs['collision_metrics'] under TEST.COLLISION_METRICS; one pass over the posed
        chunks serves both."""
        if not (self.mesh_metrics or self.collision_metrics):
            return
        out = self._mesh_metrics(f_rst, f_ref, b_ref, orient, lengths, K, scene, mesh=self.mesh_metrics,
                                 collision=self.collision_metrics)
        names = COLLISION_HYP + COLLISION_REF
        if self.mesh_metrics:
            rs["mesh_metrics"] = {n: v for n, v in out.items() if n not in names}
        if self.collision_metrics:
            rs["collision_metrics"] = {n: out[n] for n in names}

    # ------------------------------------------------------------------ K hypotheses per sequence in one pass
    MAX_SAMPLE_ROWS = 512          # the largest sampling batch that has a cluster plan (one CU per sample above it)

    @staticmethod
    def _check_num_hypotheses(k, what: str) -> int:
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= K_MAX:
            raise ValueError(f"{what} must be an integer in 1..{K_MAX}, got {k!r}")
        return k

    @classmethod
    def _row_chunks(cls, rows: int):
        """[lo, hi) ranges of at most MAX_SAMPLE_ROWS rows, evenly sized."""
        n = -(-rows // cls.MAX_SAMPLE_ROWS)
        size = -(-rows // n)
        return [(lo, min(lo + size, rows)) for lo in range(0, rows, size)]

    def _diffusion_reverse_rows(self, cond_bf, rows: int, latents=None, step_noise=None):
        """_diffusion_reverse on `rows` chains, at most MAX_SAMPLE_ROWS per launch.  cond_bf [rows or 2*rows, N, 256] batch-first
        (unconditional rows first with guidance).  The draws that are not given are made for all rows at once."""
        dev = cond_bf.device
        if latents is None:
            latents = torch.randn((rows, self.latent_dim[0], self.latent_dim[-1]), device=dev, dtype=torch.float)
        latents, eta = self._reverse_setup(latents)
        if self.scheduler.needs_noise(eta):
            steps = len(self.scheduler.timesteps)
            if step_noise is None:
                step_noise = torch.randn(steps, rows, self.latent_dim[-1], device=dev, dtype=torch.float32)
            step_noise = step_noise.reshape(steps, rows, self.latent_dim[-1])
        else:
            step_noise = None
        cfg = self.do_classifier_free_guidance
        out = []
        for lo, hi in self._row_chunks(rows):
            c = torch.cat([cond_bf[lo:hi], cond_bf[rows + lo:rows + hi]], dim=0) if cfg else cond_bf[lo:hi]
            out.append(self.denoiser.sample_loop(latents[lo:hi], c.contiguous(), self.scheduler, eta=eta,
                                                 guidance_scale=self.guidance_scale if cfg else 1.0,
                                                 step_noise=None if step_noise is None else step_noise[:, lo:hi]))
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)            # [1,rows,256]

    def _decode_rows(self, z, lengths, K, min_len, betas, orient=None, start=None):
        """Decode, renorm and pose the B*K latents z [1,B*K,256] (row b*K + k), at most MAX_SAMPLE_ROWS rows at a time: (f_rst
        [B*K,min_len,F] renormed, zeros past what a chunk decodes, joints [B*K,min_len,24,3]).  betas [B,min_len,10] and orient
        [B,min_len,3] or None are per sequence.  Every chunk is decoded before the first is posed; `start`, the time.time() at which
        the caller's pass began, puts the time up to there into self.times (encode + sample + decode, mld.py:1367-1368)."""
        rows, dev = z.shape[1], z.device
        lengths_k = [l for l in lengths for _ in range(K)]
        f_rst = torch.zeros(rows, min_len, self.vae.nfeats, device=dev, dtype=torch.float32)
        joints = torch.empty(rows, min_len, 24, 3, device=dev, dtype=torch.float32)
        chunks = self._row_chunks(rows)
        decoded = [self.vae.decode(z[:, lo:hi], lengths_k[lo:hi]) for lo, hi in chunks]
        if start is not None:
            self.times.append(time.time() - start)
        for (lo, hi), feats_c in zip(chunks, decoded):                      # feats_c [n, max length of the chunk, F], zeros past each length
            tc = min(min_len, feats_c.shape[1])
            if tc == min_len:
                fc = feats_c[:, :min_len].contiguous()
            else:
                fc = torch.zeros(hi - lo, min_len, feats_c.shape[-1], device=dev, dtype=torch.float32)
                fc[:, :tc] = feats_c[:, :tc]
            fc = self.renorm(fc)
            seq = torch.arange(lo, hi, device=dev) // K
            f_rst[lo:hi] = fc
            joints[lo:hi] = self._feats_to_joints(fc, betas[seq], orient=None if orient is None else orient[seq])
        return f_rst, joints

    def _ego_eval_hypotheses(self, batch, int_gt, K, latents=None, want_vertices=False, cond_noise=None, step_noise=None, select="first"):
        """ego_eval for K > 1 (`int_gt`: what ego_eval split off the batch under TEST.POSE_ESTIMATION_TASK).  Once per SEQUENCE: the
        PointNet scene code and its token (and the zero-scene token under guidance), the image token, vae.encode_dist of the
        interactee (and of the zero motion), the reference and interactee joints.  Per HYPOTHESIS: the posterior draw of the
        condition token, the initial latent, the DDPM step noise, decode, renorm, SMPL joints.
        Rows are sequence-major (b*K + k).  The keys of the K = 1 result are filled from hypothesis 0, or with select 'medoid' from
        the medoid of the K draws of each sequence (hm gains PAIR_DIST, medoid_index and selected_index)."""
        eps_c, eps_u = cond_noise if isinstance(cond_noise, (tuple, list)) else (cond_noise, None)
        feats_ref, transl, beta, utils_, scene, images, length, _ = split_batch(self.condition, batch)
        B = feats_ref.shape[0]
        scene_tok, img_tok = self._condition_tokens(scene, images, K, "ego_eval")
        feats_ref, transl, beta = feats_ref.float(), transl.float(), beta.float()
        lengths = length.long().reshape(-1).tolist()
        idx_ref = 0 if self.estimate == "wearer" else 1
        start = time.time()
        if self.stage in ("diffusion", "vae_diffusion"):
            f_int = self._wearer_features(feats_ref, transl, 1) if "interactee" in self.condition else None
            cond_bf = self._condition_rows(f_int, lengths, eps_c, eps_u, scene_tok, img_tok, K)      # [B*K or 2*B*K, N, 256]
            z = self._diffusion_reverse_rows(cond_bf, B * K, latents=latents, step_noise=step_noise)
        elif self.stage == "vae":                                          # K posterior draws of the target
            z = self._posterior_draws(self._wearer_features(feats_ref, transl, idx_ref), lengths, eps_c, K)
        else:
            raise ValueError(f"Not support this stage {self.stage}!")
        if self.see_future:
            lengths = [int(i // 2) for i in lengths]
        min_len = min(feats_ref.shape[1], int(max(lengths)))
        f_ref = self.renorm(self._wearer_features(feats_ref[:, :min_len], transl[:, :, :min_len], idx_ref))
        b_ref = beta[:, idx_ref, :min_len]
        o_ref = f_ref[:, :, :3] if (self.data_type == "angle" and self.name_dataset == "egobody" and not self.pred_global_orient) else None
        dev = f_ref.device
        f_rst, joints_all = self._decode_rows(z, lengths, K, min_len, b_ref, o_ref, start=start)
        out_ref = self._feats_to_joints(f_ref, b_ref, want_vertices)
        joints_ref = out_ref[0] if want_vertices else out_ref
        joints_all = joints_all.view(B, K, min_len, 24, 3)
        f_int_r = self.renorm(self._wearer_features(feats_ref[:, :min_len], transl[:, :, :min_len], 1))
        joints_int = self._feats_to_joints(f_int_r, beta[:, 1, :min_len])
        joints_int_gt = self._interactee_gt_joints(int_gt, beta, min_len)
        q_ref = self._orientation_quat(f_ref)
        q_all = self._orientation_quat(f_rst, None if o_ref is None else o_ref.repeat_interleave(K, dim=0))      # [B*K*T,4]
        # per-hypothesis errors and the diversity of the K draws: one pass of seeme_hyp_metrics over the joints
        hm = hyp_metrics_hip(joints_all, joints_ref, lengths)
        lens = torch.as_tensor(lengths, device=dev).reshape(B)
        if q_all is not None:
            mask = (torch.arange(min_len, device=dev)[None, :] < lens[:, None]).to(torch.float32).repeat_interleave(K, dim=0)
            q_ref_k = q_ref.reshape(B, min_len, 4).repeat_interleave(K, dim=0)
            hm["HEAD_ORIENTATION_ERROR"] = EgoMetrics.head_orientation_error(q_all, q_ref_k, mask, lens.repeat_interleave(K)).reshape(B, K)
        else:
            hm["HEAD_ORIENTATION_ERROR"] = torch.zeros(B, K, device=dev, dtype=torch.float32)
        hm["have_quat"] = q_all is not None
        # (the 'test' inclusion rule; allsplit_step, which knows the split, puts the 'val' rule's index there on 'val')
        hm["best_index"] = best_index(hm["MPJPE"], keep_mask(hm, "test", hm["have_quat"]))
        if select == "medoid":              # label-free choice: one seeme_hyp_pairdist pass over the same joints
            hm.update(hyp_pairdist_hip(joints_all, lengths))
            hm["selected_index"] = select_index(hm, select)
            rows = torch.arange(B, device=dev)
            pick = lambda t: t[rows, hm["selected_index"]].contiguous()              # [B,K,...] -> [B,...]
        else:
            pick = lambda t: t[:, 0].contiguous()
        f_rst0 = pick(f_rst.view(B, K, min_len, -1))
        rs = {"m_ref": f_ref, "m_rst": f_rst0, "joints_ref": joints_ref, "joints_rst": pick(joints_all),
              "orientation_quat_rst": None if q_all is None else pick(q_all.reshape(B, K, min_len, 4)).reshape(-1, 4),
              "orientation_quat_ref": q_ref,
              "root_interactee": joints_int[:, :, 0], "joints_interactee": joints_int,
              "orientation_quat_int": self._orientation_quat(f_int_r), "joints_interactee_gt": joints_int_gt, "lengths": lengths,
              "list_names": {}, "lat_t": pick(z.view(B, K, -1))[None],
              "joints_rst_all": joints_all, "m_rst_all": f_rst.view(B, K, min_len, -1), "lat_t_all": z, "hyp_metrics": hm}
        self._add_mesh_results(rs, f_rst, f_ref, b_ref, o_ref, lengths, K, scene)
        if self.social_metrics:
            rs["social_metrics"] = social_metrics_hip(joints_all, joints_ref, joints_int, q_all, q_ref, rs["orientation_quat_int"], lengths)
        if want_vertices:                                                   # meshes of the selected hypothesis only (6890 vertices per frame)
            rs["vertices_ref"] = out_ref[1]
            rs["vertices_rst"] = self._feats_to_joints(f_rst0, b_ref, True, orient=o_ref)[1]
        return rs

    # ------------------------------------------------------------------ estimation without labels
    @torch.no_grad()
    def predict(self, batch, num_hypotheses=None, betas=None, latents=None, cond_noise=None, step_noise=None):
        """K hypotheses of the wearer's motion per sequence from the conditions alone.  `batch` has the data module's tuple layout
        (``split_batch``); the WEARER's slot (index 0) of its motion, transl and beta tensors is never read and may hold anything.
        Stages 'diffusion' and 'vae_diffusion' only: stage 'vae' reconstructs its target and so needs labels.  The restrictions of
        ``ego_eval`` hold (no image condition with guidance, K <= 32), and so do its injection points (rows b*K + k, also for K = 1).
        The prediction is posed with betas [B,10] (zeros when not given) and its OWN global orientation: TEST.GLOBAL_ORIENT_PRED
        false would need the reference's.

        Returns m_rst_all [B,K,T,F] (renormed), joints_rst_all [B,K,T,24,3], lat_t_all [1,B*K,256], lengths, and hyp_metrics with
        PAIR_DIST [B,K,K] and medoid_index [B] of ``hyp_pairdist_hip`` -- what can be said about K draws without ground truth."""
        K = self.num_hypotheses if num_hypotheses is None else self._check_num_hypotheses(num_hypotheses, "num_hypotheses")
        if self.stage not in ("diffusion", "vae_diffusion"):
            raise ValueError(f"predict: stage {self.stage!r} reconstructs its target and needs labels; it runs with stage 'diffusion' or "
                             "'vae_diffusion'")
        eps_c, eps_u = cond_noise if isinstance(cond_noise, (tuple, list)) else (cond_noise, None)
        feats_ref, transl, beta, utils_, scene, images, length, _ = split_batch(self.condition, batch)
        B = feats_ref.shape[0]
        scene_tok, img_tok = self._condition_tokens(scene, images, K, "predict")
        lengths = length.long().reshape(-1).tolist()
        dev = feats_ref.device
        f_int = None
        if "interactee" in self.condition:
            # the interactee's slot only: _wearer_features(.., 1) slices person 1 out of the motion and the translation
            # (cut to the longest sequence: the encoder builds its mask from max(lengths) -- a lone last window may be shorter than T)
            n_enc = min(int(feats_ref.shape[1]), int(max(lengths)))
            f_int = self._wearer_features(feats_ref[:, :n_enc, 1:2].float(), transl[:, 1:2, :n_enc].float(), 0)
        cond_bf = self._condition_rows(f_int, lengths, eps_c, eps_u, scene_tok, img_tok, K)
        z = self._diffusion_reverse_rows(cond_bf, B * K, latents=latents, step_noise=step_noise)
        if self.see_future:
            lengths = [int(i // 2) for i in lengths]
        min_len = min(feats_ref.shape[1], int(max(lengths)))
        if betas is None:
            betas = torch.zeros(B, 10, device=dev, dtype=torch.float32)
        betas = torch.as_tensor(betas, device=dev, dtype=torch.float32)
        if tuple(betas.shape) != (B, 10):
            raise ValueError(f"predict: betas are {tuple(betas.shape)}: expected [B,10] = [{B},10]")
        f_rst, joints_all = self._decode_rows(z, lengths, K, min_len, betas[:, None, :].expand(B, min_len, 10))
        joints_all = joints_all.view(B, K, min_len, 24, 3)
        return {"m_rst_all": f_rst.view(B, K, min_len, -1), "joints_rst_all": joints_all, "lat_t_all": z, "lengths": lengths,
                "hyp_metrics": hyp_pairdist_hip(joints_all, lengths)}

    @torch.no_grad()
    def estimate_interactee(self, crops_or_feats, scene_views_or_feats, center, scale, intrinsics, z=None, num_samples: int = 1,
                            generator=None):
        """The interactee from what a headset records, in the image's OpenCV camera frame (``ProHMRScene.forward_step`` without its
        losses, prohmr_scene.py:108-233).  crops_or_feats: uint8 [L,224,224,3] / float32 [L,3,224,224] crops cut by
        ``prohmr_head.head_box`` (needs model.image_backbone) or pooled features [L,2048]; scene_views_or_feats: clouds [L,P,3] in
        the camera frame (needs a 'scene' condition) or features [L,512]; center [L,2], scale [L]; intrinsics (f, cx, cy) in pixels,
        [3] or [L,3].  z [L,S,144] or, without it, sample 0 = the mode and num_samples - 1 draws of `generator`.
        -> dict: pose6d [L,S,144], rotmat [L,S,24,3,3], betas [L,10], cam [L,3], log_prob [L,S], transl [L,3], ctx [L,2566]."""
        from . import prohmr_head as PH
        if not self.interactee_head:
            raise NotImplementedError("estimate_interactee needs the pose head: set model.interactee_head: true (INTEGRATION.md N)")
        dev = self.proscene.flow.fc_head.init_cam.device
        x = crops_or_feats.to(dev)
        if x.dim() == 4:
            if not self.image_backbone:
                raise NotImplementedError("estimate_interactee was given crops, and the ResNet-50 backbone is off: set "
                                          "model.image_backbone: true or pass its pooled features [L,2048]")
            x = self.proscene.encode_image(x)
        sc = scene_views_or_feats.to(dev)
        if sc.dim() == 3:
            if "scene" not in self.condition:
                raise NotImplementedError("estimate_interactee was given scene clouds, and the model has no scene encoder ('scene' is "
                                          "not in model.condition): pass its features [L,512]")
            sc = self.proscene.encode_scene(sc.float().contiguous())
        n = x.shape[0]
        intr = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev)
        intr = intr.expand(n, 3) if intr.dim() == 1 else intr
        if tuple(intr.shape) != (n, 3):
            raise ValueError(f"intrinsics are {tuple(intr.shape)}: expected [3] or [{n},3] = (f, cx, cy)")
        center = torch.as_tensor(center, dtype=torch.float32, device=dev)
        scale = torch.as_tensor(scale, dtype=torch.float32, device=dev)
        ctx = PH.context_rows(x.float(), sc.float(), center, scale, intr[:, 0], intr[:, 1], intr[:, 2])
        if z is None:
            z = PH.draw_z(n, int(num_samples), generator, dev)
        pose6d, rotmat, betas, cam, log_prob = PH.flow_head_hip(self.proscene.flow, ctx, z.to(dev, torch.float32))
        transl = PH.cam_to_transl(cam, center, scale, intr[:, 0], intr[:, 1], intr[:, 2])
        return {"pose6d": pose6d, "rotmat": rotmat, "betas": betas, "cam": cam, "log_prob": log_prob, "transl": transl, "ctx": ctx}

    @torch.no_grad()
    def predict_recording(self, batch_of_windows, n_frames, overlap=None, betas=None, medoid_weight=None, num_hypotheses=None,
                          latents=None, cond_noise=None, step_noise=None, window_frames=None, head_path=None, head_weight=None,
                          head_anchor=None, anchor_sigma=None, scene_cloud=None, scene_weight=None, scene_report=None, capsules=None,
                          head_rot=None, head_rot_weight=None, head_rot_report=None, head_offset=None):
        """One motion for a recording of `n_frames` frames.  The batch rows are its W windows (``recording.window_plan`` of n_frames,
        the batch's T and `overlap`; ``recording.windows_batch`` builds them), all in ONE coordinate frame unless `window_frames` says
        otherwise: the seam cost compares global joint positions (GIMO scenes are in one frame already; a moving camera: below).  Steps: ``predict`` (K hypotheses per window) -> ``overlap_cost`` -> unary[w,k] = medoid_weight x
        sum_j PAIR_DIST[w,k,j] / max(K-1, 1) -> ``path_select`` -> the chosen features -> ``stitch_windows`` -> SMPL joints.

        overlap: None = TEST.WINDOW_OVERLAP, and T // 4 without it.  medoid_weight: None = TEST.PATH_MEDOID_WEIGHT (1.0); 0 passes no
        unary term, the path then follows the seams alone.  betas [10] or [W,10] pose every window and the stitched motion.

        Returns motion [n_frames,F] (renormed), joints [n_frames,24,3], path [W], seam_cost [W-1] (mm: the disagreement of the two
        chosen hypotheses on the frames a seam shares), path_cost, window_starts, window_lengths and ``predict``'s result.

        window_frames [W,4,4]: every window is in a frame of its OWN, M_w mapping the common (world) frame to window w's
        (``recording.windows_batch`` with world2cam).  The hypotheses' joints are then brought to the world frame by the inverse of
        M_w before the seams are compared, the chosen windows' features are re-framed the same way (the orientation, and the
        translation when the features carry it: ``recording.reframe_smpl`` / ``reframe_rot6d``) before they are stitched, and motion,
        joints and seam_cost are in the world frame; ``predict``'s result stays in the windows' frames and the result gains
        window_frames.  The medoid term is invariant under a rigid map and is taken as it is.

        head_path [n_frames,3]: the headset's position in every frame, in the frame the seams are compared in (the world frame with
        window_frames; ``recording.camera_centres``).  Given alone it changes nothing.  head_weight (None = TEST.PATH_HEAD_WEIGHT, 0)
        > 0 adds head_weight x ``head_path_cost`` (mm: how far a hypothesis' head strays from the shape of the headset's path over
        its window) to the unary; the result gains head_cost [W,K] and head_cost_path [W].  It needs features that carry a
        translation: other hypotheses have no global position to compare.  head_anchor (None = TEST.HEAD_ANCHOR, false) shifts the
        stitched motion's head onto the path: shift, residual = ``head_anchor`` of the stitched joints with the taps of anchor_sigma
        (None = TEST.HEAD_ANCHOR_SIGMA); joints and, where the features carry one, the motion's translation move by shift, and the
        result gains head_shift [n_frames,3], head_residual [n_frames] (mm) and transl [n_frames,3] (the motion's translation, or
        the shift alone for features without one).

        head_rot [n_frames,3,3]: the headset's orientation in every frame, the rotation device -> the frame the seams are compared in
        (``recording.camera_rotations`` of world2cam, or the recording's head_rot).  Given alone it changes nothing and launches
        nothing.  head_rot_weight (None = TEST.PATH_HEAD_ROT_WEIGHT, 0) > 0 adds head_rot_weight x the cost of
        ``recording.head_rot_cost_hip`` (degrees: how far a hypothesis' head turns against the device over its window, a constant
        mount rotation removed; the weight is mm per degree and no value has been measured) to the unary.  It reads the features'
        joint rotations alone (m_rst_all, in the windows' own frames, against ``recording.head_rot_windows`` with window_frames), so
        it serves every layout, rot6d and features without a translation included; the result gains head_rot_cost [W,K] and
        head_rot_cost_path [W].  head_rot_report (None = TEST.HEAD_ROT_REPORT, false) runs the kernel once on the stitched motion as
        one row of n_frames frames; the result gains head_rot_residual [n_frames] (degrees per frame from the recording's one mean
        mount rotation) and head_rot_mean (their mean).  head_offset [3] (None = TEST.HEAD_DEVICE_OFFSET, zeros): the vector from
        joint 15 to the device in the device's frame, metres (``recording.fit_device_offset``).  When it is not zero, head_path is
        replaced by ``recording.head_joint_path`` (head_path[n] - C_n offset, the lever arm, which turns with the head) before
        head_weight and head_anchor use it; it needs head_rot.

        scene_cloud [N,3]: the scene's points in the frame the seams are compared in (the world frame with window_frames).  Given
        alone it changes nothing and launches nothing.  scene_weight (None = TEST.PATH_SCENE_WEIGHT, 0) > 0 adds scene_weight x the
        cost of ``recording.scene_depth_hip`` (mm: how deep the capsules round a hypothesis' bones reach into the cloud, the mean
        over its window) to the unary; the result gains scene_cost [W,K], scene_hits [W,K] (frames that penetrate) and
        scene_cost_path [W].  Like head_weight it needs features that carry a translation.  scene_report (None = TEST.SCENE_REPORT,
        false) runs the same kernel on the final joints (after the anchoring, if any) as one row of n_frames frames; the result
        gains scene_depth [n_frames] (mm).  capsules: (segs [NB,2], radius [NB]); None = ``recording.body_capsules`` of the model's
        SMPL with the betas and TEST.SCENE_CAPSULE_QUANTILE (0.5).  The proxy leaves out the feet, the skull above joint 15 and the
        interactee's body, and a cloud only holds what was seen."""
        from . import recording as R
        from .track import gaussian_taps
        feats_ref, _t, _b, _u, _s, _i, length, _ = split_batch(self.condition, batch_of_windows)
        W, T = int(feats_ref.shape[0]), int(feats_ref.shape[1])
        O = overlap if overlap is not None else (self.window_overlap if self.window_overlap is not None else T // 4)
        if self.see_future:
            raise NotImplementedError("predict_recording with TEST.SEE_FUTURE: the windows are then half as long as the plan assumes")
        starts, lens = R.window_plan(n_frames, T, O)
        if len(starts) != W or length.long().reshape(-1).tolist() != lens:
            raise ValueError(f"predict_recording: the batch has {W} windows of lengths {length.long().reshape(-1).tolist()}, but the plan "
                             f"of n_frames {n_frames}, T {T}, overlap {O} is {lens}")
        mw = self.path_medoid_weight if medoid_weight is None else medoid_weight
        if isinstance(mw, bool) or not isinstance(mw, (int, float)) or not 0 <= mw < float("inf"):
            raise ValueError(f"medoid_weight must be a finite number >= 0, got {mw!r}")
        dev = feats_ref.device
        hw = self.path_head_weight if head_weight is None else head_weight
        if isinstance(hw, bool) or not isinstance(hw, (int, float)) or not 0 <= hw < float("inf"):
            raise ValueError(f"head_weight must be a finite number >= 0, got {hw!r}")
        anchor = self.head_anchor if head_anchor is None else head_anchor
        if not isinstance(anchor, bool):
            raise ValueError(f"head_anchor must be true or false, got {anchor!r}")
        sigma = self.head_anchor_sigma if anchor_sigma is None else check_sigma(anchor_sigma, "anchor_sigma")
        if (hw > 0 or anchor) and head_path is None:
            raise ValueError("predict_recording: head_weight > 0 and head_anchor need head_path [n_frames,3], the headset's position in "
                             "every frame (recording.camera_centres of world2cam, or the recording's head_path)")
        if hw > 0 and not self.transl_in_feats:
            raise ValueError("predict_recording: head_weight (TEST.PATH_HEAD_WEIGHT) > 0 needs features that carry a translation "
                             "(TRAIN.ABLATION.PREDICT_TRANSL, not rot6d): these hypotheses have no global position to compare with the "
                             "headset's path; head_anchor places them")
        hrw = self.path_head_rot_weight if head_rot_weight is None else head_rot_weight
        if isinstance(hrw, bool) or not isinstance(hrw, (int, float)) or not 0 <= hrw < float("inf"):
            raise ValueError(f"head_rot_weight must be a finite number >= 0, got {hrw!r}")
        rot_report = self.head_rot_report if head_rot_report is None else head_rot_report
        if not isinstance(rot_report, bool):
            raise ValueError(f"head_rot_report must be true or false, got {rot_report!r}")
        offset = self.head_device_offset if head_offset is None else check_head_offset(head_offset, "head_offset")
        lever = bool((offset != 0).any())
        if (hrw > 0 or rot_report or lever) and head_rot is None:
            raise ValueError("predict_recording: head_rot_weight > 0, head_rot_report and a head_offset that is not zero need head_rot "
                             "[n_frames,3,3], the headset's orientation in every frame (the recording's head_rot, or "
                             "recording.camera_rotations of world2cam)")
        rot = R.check_head_rot(head_rot, n_frames, "predict_recording") if hrw > 0 or rot_report or lever else None
        rot_layout = R.stitch_layout(self.data_type, self.transl_in_feats)
        sw = self.path_scene_weight if scene_weight is None else scene_weight
        if isinstance(sw, bool) or not isinstance(sw, (int, float)) or not 0 <= sw < float("inf"):
            raise ValueError(f"scene_weight must be a finite number >= 0, got {sw!r}")
        report = self.scene_report if scene_report is None else scene_report
        if not isinstance(report, bool):
            raise ValueError(f"scene_report must be true or false, got {report!r}")
        if (sw > 0 or report) and scene_cloud is None:
            raise ValueError("predict_recording: scene_weight > 0 and scene_report need scene_cloud [N,3], the scene's points in the "
                             "frame the seams are compared in (the recording's scene_vertices, or its scene)")
        if sw > 0 and not self.transl_in_feats:
            raise ValueError("predict_recording: scene_weight (TEST.PATH_SCENE_WEIGHT) > 0 needs features that carry a translation "
                             "(TRAIN.ABLATION.PREDICT_TRANSL, not rot6d): these hypotheses have no global position to compare with the "
                             "scene's points")
        cloud = None
        if scene_cloud is not None and (sw > 0 or report):
            cloud = torch.as_tensor(scene_cloud)
            if cloud.dim() != 2 or cloud.shape[1] != 3 or cloud.shape[0] < 1 or not cloud.dtype.is_floating_point:
                raise ValueError(f"predict_recording: scene_cloud is {tuple(cloud.shape)} {cloud.dtype}: expected floats [N,3], N >= 1")
            cloud = cloud.to(device=dev, dtype=torch.float32).contiguous()
        hp = None
        if head_path is not None:
            hp = torch.as_tensor(head_path)
            if tuple(hp.shape) != (n_frames, 3) or not hp.dtype.is_floating_point:
                raise ValueError(f"predict_recording: head_path is {tuple(hp.shape)} {hp.dtype}: expected floats [n_frames,3] = "
                                 f"[{n_frames},3]")
            if lever:                                                          # the device's path -> the path of joint 15 itself
                hp = torch.from_numpy(R.head_joint_path(hp, rot, offset))
            hp = hp.to(device=dev, dtype=torch.float32).contiguous()
        if betas is not None:
            betas = torch.as_tensor(betas, device=dev, dtype=torch.float32)
            if betas.dim() == 1:
                betas = betas[None].expand(W, 10)
        pr = self.predict(batch_of_windows, num_hypotheses=num_hypotheses, betas=betas, latents=latents, cond_noise=cond_noise,
                          step_noise=step_noise)
        K = int(pr["m_rst_all"].shape[1])
        jts = pr["joints_rst_all"]
        if window_frames is not None:
            Mw = torch.as_tensor(window_frames, device=dev)
            if tuple(Mw.shape) != (W, 4, 4):
                raise ValueError(f"predict_recording: window_frames are {tuple(Mw.shape)}: expected [W,4,4] = [{W},4,4]")
            Ai, ai = R.rigid_parts(R.rigid_inverse(Mw.double()).float())            # window frame -> world
            b0 = torch.zeros(W, 10, device=dev, dtype=torch.float32)               # (rot6d is posed with zero betas)
            J0 = R.rest_pelvis(self.smpl_model, b0 if betas is None or self.data_type == "rot6d" else betas)
            jts = R.reframe_joints(jts, J0[:, None, None], Ai[:, None, None], ai[:, None, None], self.transl_in_feats).contiguous()
        # (a single window shorter than T comes back from predict cut to its length; it has no seam, and the stitch gets it padded)
        cost = R.overlap_cost_hip(jts, O) if W > 1 else torch.zeros(0, K, K, device=dev, dtype=torch.float32)
        unary = None
        if mw > 0:
            unary = (float(mw) / max(K - 1, 1)) * pr["hyp_metrics"]["PAIR_DIST"].sum(dim=2)
        head_cost = None
        if hw > 0:                                                             # (jts: the frame the path is in)
            head_cost = R.head_path_cost_hip(jts.contiguous(), R.head_path_windows(hp, starts, lens, int(jts.shape[2])), lens)
            unary = float(hw) * head_cost if unary is None else unary + float(hw) * head_cost
        head_rot_cost = None
        if hrw > 0:                                                            # (m_rst_all: the windows' own frames)
            dq = R.head_rot_windows(rot, starts, lens, int(pr["m_rst_all"].shape[2]), window_frames=Mw if window_frames is not None else None)
            head_rot_cost = R.head_rot_cost_hip(pr["m_rst_all"].contiguous(), rot_layout, dq.to(dev), lens)["cost"]
            unary = float(hrw) * head_rot_cost if unary is None else unary + float(hrw) * head_rot_cost
        scene = None
        if cloud is not None:
            if capsules is None:                                               # (rot6d is posed with zero betas)
                capsules = R.body_capsules(self.smpl_model, None if betas is None or self.data_type == "rot6d" else betas[0],
                                           float(self.scene_capsule_quantile))
            if not isinstance(capsules, (tuple, list)) or len(capsules) != 2:
                raise ValueError("predict_recording: capsules must be (segs [NB,2], radius [NB])")
        if sw > 0:                                                             # (jts: the frame the cloud is in)
            scene = R.scene_depth_hip(jts.contiguous(), lens, cloud, capsules[0], capsules[1])
            unary = float(sw) * scene["cost"] if unary is None else unary + float(sw) * scene["cost"]
        sel = R.path_select_hip(cost, unary)
        chosen = pr["m_rst_all"][torch.arange(W, device=dev), sel["path"]].contiguous()          # [W,T,F]
        if window_frames is not None:
            if self.data_type == "rot6d":
                chosen[..., :6] = R.reframe_rot6d(chosen[..., :6], Ai[:, None])
            else:
                tr = chosen[..., -3:] if self.transl_in_feats else torch.zeros_like(chosen[..., :3])
                go_w, tr_w = R.reframe_smpl(chosen[..., :3], tr, J0[:, None], Ai[:, None], ai[:, None])
                chosen[..., :3] = go_w
                if self.transl_in_feats:
                    chosen[..., -3:] = tr_w
        if chosen.shape[1] < T:
            chosen = torch.nn.functional.pad(chosen, (0, 0, 0, T - chosen.shape[1]))
        motion = R.stitch_windows_hip(chosen, O, n_frames, R.stitch_layout(self.data_type, self.transl_in_feats))
        b1 = betas[:1] if betas is not None else torch.zeros(1, 10, device=dev, dtype=torch.float32)
        joints = self._feats_to_joints(motion[None], b1[:, None, :].expand(1, n_frames, 10))[0]
        out = {"motion": motion, "joints": joints, "path": sel["path"], "seam_cost": sel["seam_cost"], "path_cost": sel["path_cost"],
               "window_starts": starts, "window_lengths": lens, "predict": pr}
        if window_frames is not None:
            out["window_frames"] = Mw
        if head_cost is not None:
            out["head_cost"] = head_cost
            out["head_cost_path"] = head_cost[torch.arange(W, device=dev), sel["path"]]
        if anchor:
            shift, residual = R.head_anchor_hip(joints.contiguous(), hp, gaussian_taps(sigma))
            out["joints"] = joints + shift[:, None]
            if self.transl_in_feats:
                motion[:, -3:] += shift
            out["head_shift"], out["head_residual"] = shift, residual
            out["transl"] = motion[:, -3:].clone() if self.transl_in_feats else shift
        if head_rot_cost is not None:
            out["head_rot_cost"] = head_rot_cost
            out["head_rot_cost_path"] = head_rot_cost[torch.arange(W, device=dev), sel["path"]]
        if rot_report:                                                         # the stitched motion as one row of n_frames frames
            turned = R.head_rot_cost_hip(motion[None, None].contiguous(), rot_layout, R.head_rot_windows(rot, [0], [n_frames], n_frames).to(dev),
                                         [n_frames])
            out["head_rot_residual"], out["head_rot_mean"] = turned["angle"][0, 0], turned["cost"][0, 0]
        if scene is not None:
            out["scene_cost"], out["scene_hits"] = scene["cost"], scene["hits"]
            out["scene_cost_path"] = scene["cost"][torch.arange(W, device=dev), sel["path"]]
        if report:                                                             # the final joints as one row of n_frames frames
            out["scene_depth"] = R.scene_depth_hip(out["joints"].contiguous()[None, None], [n_frames], cloud, capsules[0],
                                                   capsules[1])["depth"][0, 0]
        return out

    def forward(self, batch, **kw):
        return self.ego_eval(batch, **kw)

    sample = forward

    # ------------------------------------------------------------------ step dispatch (mld.py:2037-2130, base.py:38-53)
    def allsplit_step(self, split: str, batch, batch_idx=0):
        loss = None
        if split in ("train", "val"):
            if self.stage == "vae":
                rs_set = self.train_vae_forward(batch)
            elif self.stage == "diffusion":
                rs_set = self.train_diffusion_forward(batch)
            else:
                raise ValueError(f"Not support this stage {self.stage}!")
            loss = self.losses[split].update(rs_set)
        if split in ("val", "test"):
            rs_set = self.ego_eval(batch)
            self.EgoMetric.update(rs_set["joints_rst"], rs_set["joints_ref"], rs_set["lengths"],
                                  rs_set.get("orientation_quat_rst"), rs_set.get("orientation_quat_ref"), split=split,
                                  jts_int=rs_set.get("joints_interactee"), jts_int_gt=rs_set.get("joints_interactee_gt"))
            if "hyp_metrics" in rs_set:                                    # TEST.NUM_HYPOTHESES > 1
                hm = rs_set["hyp_metrics"]
                if split != "test":
                    hm["best_index"] = best_index(hm["MPJPE"], keep_mask(hm, split, hm["have_quat"]))
                self.HypMetric.update(hm, split)
                if "selected_index" in hm:                                 # TEST.HYP_SELECT medoid
                    self.SelMetric.update(hm, split, rs_set.get("mesh_metrics"))
            if "mesh_metrics" in rs_set:                                   # TEST.MESH_METRICS
                if "hyp_metrics" in rs_set:
                    hm = rs_set["hyp_metrics"]
                    keep = keep_mask(hm, split, hm["have_quat"])
                else:                                                      # K = 1: the same rule on this batch's per-sequence errors
                    q_rst, q_ref = rs_set.get("orientation_quat_rst"), rs_set.get("orientation_quat_ref")
                    per = EgoMetrics.per_sequence(rs_set["joints_rst"], rs_set["joints_ref"], rs_set["lengths"], q_rst, q_ref)
                    keep = keep_mask({k: v[:, None] for k, v in per.items()}, split, q_rst is not None and q_ref is not None)
                self.MeshMetric.update(rs_set["mesh_metrics"], keep)
            if "collision_metrics" in rs_set:                              # TEST.COLLISION_METRICS
                self.CollMetric.update(rs_set["collision_metrics"])
            if "social_metrics" in rs_set:                                 # TEST.SOCIAL_METRICS
                if "hyp_metrics" in rs_set:
                    hm = rs_set["hyp_metrics"]
                    mp, root, keep = hm["MPJPE"], hm["ROOT_ERROR"], keep_mask(hm, split, hm["have_quat"])
                else:                                                      # K = 1: the sequences EgoMetrics.update counts for MPJPE
                    per = {k: v[:, None] for k, v in EgoMetrics.per_sequence(
                        rs_set["joints_rst"], rs_set["joints_ref"], rs_set["lengths"], rs_set["orientation_quat_rst"],
                        rs_set["orientation_quat_ref"]).items()}
                    mp, root, keep = per["MPJPE"], per["ROOT_ERROR"], keep_mask(per, split, True)
                self.SocialMetric.update(rs_set["social_metrics"], mp, root, keep)
        if split == "test":
            return rs_set["joints_rst"]
        return loss

    def training_step(self, batch, batch_idx=0):
        return self.allsplit_step("train", batch, batch_idx)

    def validation_step(self, batch, batch_idx=0):
        return self.allsplit_step("val", batch, batch_idx)

    def test_step(self, batch, batch_idx=0):
        return self.allsplit_step("test", batch, batch_idx)

    def capture_training_step(self, batch, warmup: int = 3):
        """One stage-2 training step (frozen HIP encoders, denoiser forward + backward, AdamW) captured as ONE
        hipGraph on static input buffers -- the launch-bound chain of small kernels replays without host work.
        Returns replay(new_batch=None) -> loss tensor (static).  The AdamW update in the graph is the one-launch
        ``seeme_adamw_step_dev`` on the existing optimiser's state (step count and learning rate live on the device, so
        replays advance them and an LR-scheduler edit reaches the graph); with data parallelism the graph ends after
        backward and the gradient all-reduce + optimiser step stay eager after the replay."""
        from . import distributed as D
        world = D.world()[1]
        self.configure_optimizers()
        fused = getattr(self, "_fused_adamw", None)
        if fused is None:
            raise NotImplementedError("capture_training_step needs the one-launch AdamW (TRAIN.FUSED_ADAMW, ROCm parameters): "
                                      "torch.optim.AdamW built with capturable=False cannot be stepped inside a capture")
        if self.stage != "diffusion":
            raise NotImplementedError("capture_training_step: stage 'diffusion'")
        static = [b.clone() if torch.is_tensor(b) else b for b in batch]
        losses = self.losses["train"]

        def step():
            loss = losses.update(self.train_diffusion_forward(static), accumulate=False)
            self.backward(loss)
            if world == 1:
                fused.step(device_step=True)
            return loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            # real steps: the first discovers the parameters on the path, the next ones create the gradient bucket and the
            # optimiser's pointer tables -- all of which must exist before the capture
            for _ in range(max(3 if self.grad_bucket() is None else 1, warmup)):
                step()
                if world > 1:
                    b = self.grad_bucket()
                    D.allreduce_gradients(self._used_params) if b is None else b.allreduce()
                    self.optimizer_update()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = step()

        def replay(new_batch=None):
            if new_batch is not None:
                for dst, src in zip(static, new_batch):
                    if torch.is_tensor(dst):
                        dst.copy_(src)
            if world == 1:
                fused.sync_lr()
            graph.replay()
            if world > 1:
                self.grad_bucket().allreduce()
                self.optimizer_update()
            else:
                fused.note_replay()
            return static_loss

        return replay

    def grad_bucket(self):
        """The flat gradient buffer (distributed.GradBucket) of the parameters that RECEIVE gradients -- known after the
        first backward, which runs on separate tensors (a parameter off the path, e.g. denoiser.mem_pos.pe, keeps
        ``.grad`` None for ever, so AdamW never decays it, as in the reference) -- laid out around the HIP backward's own
        gradient block when stage 2 trains through it; rebuilt when that block is re-created.  None before that first step."""
        from . import distributed as D
        used = getattr(self, "_used_params", None)
        if used is None:
            return None
        pack = getattr(self.denoiser, "_train_pack", None) if self.stage == "diffusion" and self.hip_backward else None
        b = getattr(self, "_bucket", None)
        if b is None or not b.matches(pack):
            b = D.GradBucket(used, pack)
            self._bucket = b
        return b

    def backward(self, loss):
        """loss.backward() into the flat bucket; the very first call discovers which parameters are on the path.
        Returns the bucket (None on the discovery step)."""
        b = self.grad_bucket()
        if b is None:
            for p in self.trainable_parameters():
                p.grad = None
            loss.backward()
            self._used_params = [p for p in self.trainable_parameters() if p.grad is not None]
        else:
            b.prepare()
            loss.backward()
        # the caller usually keeps `loss` (logging): cut it loose from the autograd graph, or the graph's AccumulateGrad nodes --
        # created on THIS stream -- stay alive and are reused by a later backward on another stream (a hipGraph capture runs on
        # a side stream: the engine then synchronises with the non-capturing stream and the capture dies in hipStreamEndCapture)
        if loss.grad_fn is not None and not torch.cuda.is_current_stream_capturing():
            loss.detach_()
        return b

    def optimizer_step(self, loss, events=None):
        """backward -> (data-parallel) gradient all-reduce -> AdamW step; what Lightning + DDP do around
        training_step in the reference (train.py:127-149).  Every gradient lives in one flat buffer, so the exchange is
        ONE all_reduce of it in place.  `events`: optional 4 torch.cuda.Event (start, after backward, after all-reduce,
        after AdamW) recorded on the current stream."""
        from . import distributed as D
        self.configure_optimizers()
        if self._ema_raw is not None:
            raise RuntimeError("optimizer_step inside ema_scope(): the parameters hold the EMA weights")
        if events is not None:
            events[0].record()
        bucket = self.backward(loss)
        if events is not None:
            events[1].record()
        if bucket is None:
            D.allreduce_gradients(self._used_params)
        else:
            bucket.allreduce()
        if events is not None:
            events[2].record()
        self.optimizer_update()
        if events is not None:
            events[3].record()
