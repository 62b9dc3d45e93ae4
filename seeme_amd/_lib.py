"""ctypes binding of libseeme_hip.so (the C-ABI declared in include/seeme_hip.h).

There is deliberately NO fallback: if the library is missing or a call fails the caller gets an
exception.  The structures below mirror the header field by field.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEEME_HIP_LIB: another build of the same library (debug builds with cycle stamps)
LIB_PATH = os.environ.get("SEEME_HIP_LIB") or os.path.join(_HERE, "libseeme_hip.so")

NLAYERS = 5
TROW = 7680
CROW = 5120
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
SCHED_NONE, SCHED_DDIM, SCHED_DDPM = 0, 1, 2

fp = C.c_void_p  # device pointers travel as integers


class SeemeError(RuntimeError):
    pass


class LinearArgs(C.Structure):
    _fields_ = [("A", fp), ("lda", C.c_int), ("A2", fp), ("lda2", C.c_int), ("K1", C.c_int),
                ("W", fp), ("ldw", C.c_int), ("bias", fp), ("res", fp), ("ldr", C.c_int),
                ("ln_w", fp), ("ln_b", fp), ("pre_ln_w", fp), ("pre_ln_b", fp),
                ("Y", fp), ("ldy", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("pre_act", C.c_int), ("act", C.c_int), ("eps", C.c_float)]


class XfLayer(C.Structure):
    _fields_ = [(n, fp) for n in ("in_w", "in_b", "out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b",
                                  "n1_w", "n1_b", "n2_w", "n2_b",
                                  "ca_in_w", "ca_in_b", "ca_out_w", "ca_out_b", "n3_w", "n3_b")]


class SkipStack(C.Structure):
    _fields_ = [("layer", XfLayer * NLAYERS), ("skip_w", fp * 2), ("skip_b", fp * 2),
                ("norm_w", fp), ("norm_b", fp)]


class XfLayerH(C.Structure):
    _fields_ = [(n, fp) for n in ("in_w", "out_w", "l1_w", "l2_w")]


class VaeWeightsH(C.Structure):
    _fields_ = [("enc", XfLayerH * NLAYERS), ("dec", XfLayerH * NLAYERS), ("enc_skip", fp * 2), ("dec_skip", fp * 2),
                ("emb_w", fp), ("fin_w", fp), ("ca_fold_w", fp), ("dec_pro", fp), ("dec_pro_T", C.c_int)]


def pack_mfma16(W, dtype):
    """[N,K] matrix -> 16-bit copy in MFMA fragment order [N/16][K/32][kq=4][r=16][8] (N padded to 16, K to 32):
    every wave-load of a B fragment is then 1 KiB contiguous."""
    import torch
    N, K = W.shape
    Np, Kp = (N + 15) // 16 * 16, (K + 31) // 32 * 32
    Wz = torch.zeros(Np, Kp, device=W.device, dtype=dtype)
    Wz[:N, :K] = W.detach().to(dtype)
    return Wz.view(Np // 16, 16, Kp // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


class VaeWeights(C.Structure):
    _fields_ = [("nfeats", C.c_int), ("ff", C.c_int), ("token", fp), ("pe_enc", fp), ("pe_dec", fp),
                ("emb_w", fp), ("emb_ldw", C.c_int), ("emb_b", fp), ("fin_w", fp), ("fin_b", fp),
                ("enc", SkipStack), ("dec", SkipStack), ("ca_fold_w", fp), ("ca_fold_b", fp), ("h16", fp)]


class DenoiserWeights(C.Structure):
    _fields_ = [("wg", fp), ("wdtype", C.c_int), ("vp", fp), ("layout", fp), ("nhead", C.c_int), ("ff_sa", C.c_int),
                ("ff", C.c_int), ("kv_cat_w", fp), ("kv_cat_b", fp), ("style_cat_w", fp), ("style_cat_b", fp),
                ("time_w1", fp), ("time_b1", fp), ("time_w2", fp), ("time_b2", fp),
                ("ca_kv_w", fp * NLAYERS), ("ca_kv_b", fp * NLAYERS),
                ("ca_tn_w", fp * NLAYERS), ("ca_tn_b", fp * NLAYERS),
                ("ca_fold_w", fp), ("ca_fold_b", fp), ("ln_ones", fp), ("ln_zeros", fp), ("sa_fold", C.c_int),
                ("ca_pn_w", fp), ("ca_pn_b", fp), ("ca_po_w", fp), ("ca_po_b", fp)]


class SampleArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("steps", C.c_int), ("sched", C.c_int), ("cfg", C.c_int),
                ("guidance_scale", C.c_float), ("latents", fp), ("ctab", fp), ("ttab", fp), ("trow", fp),
                ("trow_per_sample", C.c_int), ("coef", fp), ("noise", fp), ("out", fp), ("catab", fp), ("save", fp), ("force_query", C.c_int), ("drop", fp), ("drop_scale", C.c_float), ("xcds", C.c_int)]


class DenCluster(C.Structure):
    _fields_ = [("wgc", fp), ("wdtype", C.c_int), ("vpc", fp), ("C", C.c_int), ("placement", C.c_int), ("flags", C.c_int),
                ("xchg", fp), ("xchg_bytes", C.c_size_t), ("query", C.c_int), ("samples", C.c_int),
                ("xchg_zeroed", C.c_int)]


class SmplModel(C.Structure):
    _fields_ = [("V", C.c_int), ("v_template", fp), ("blend_w", fp), ("lbs_weights", fp), ("J_template", fp),
                ("J_shapedirs", fp), ("parents", fp), ("ex_template", fp), ("ex_shapedirs", fp),
                ("ex_posedirs", fp), ("ex_weights", fp)]


class PointnetWeights(C.Structure):
    _fields_ = [("out_dim", C.c_int), ("pos_w", fp), ("pos_b", fp), ("fc0_w", fp * 4), ("fc0_b", fp * 4),
                ("fc1_w", fp * 4), ("fc1_b", fp * 4), ("sc_w", fp * 4), ("fcc_w", fp), ("fcc_b", fp)]


class PointnetBf16(C.Structure):
    _fields_ = [("posf", fp), ("stream", fp * 4), ("sc3f", fp)]


class GlueRows(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("dist", fp), ("dist_rows", C.c_int), ("eps_z", fp), ("eps_c", fp),
                ("slot_c", C.c_int), ("cond", fp), ("noise", fp), ("timesteps", fp), ("acp", fp), ("freq", fp),
                ("flip_sin_to_cos", C.c_int), ("latents", fp), ("noisy", fp), ("tfeat", fp)]


class GemmProblem(C.Structure):
    _fields_ = [("a", fp * 10), ("b", fp * 10), ("seg_len", C.c_int * 10), ("a_ks", C.c_long * 10),
                ("b_ks", C.c_long * 10), ("nseg", C.c_int), ("a_rs", C.c_long), ("b_cs", C.c_long), ("c", fp), ("ldc", C.c_long),
                ("M", C.c_int), ("N", C.c_int), ("a_pro", C.c_int), ("a_p0", fp), ("a_p1", fp), ("b_pro", C.c_int),
                ("b_p0", fp), ("b_p1", fp), ("bias", fp), ("epi", C.c_int), ("e0", fp), ("e_ld", C.c_long),
                ("accumulate", C.c_int), ("colsum", fp), ("tile0", C.c_int), ("tiles_n", C.c_int), ("nbatch", C.c_int),
                ("a_bstride", C.c_long), ("b_bstride", C.c_long), ("c_bstride", C.c_long), ("alpha", C.c_float), ("addend", fp),
                ("add_ld", C.c_long)]


class VtLn(C.Structure):
    _fields_ = [("sub", fp), ("res", fp), ("gamma", fp), ("beta", fp), ("y", fp), ("xhat", fp), ("rstd", fp), ("M", C.c_long),
                ("sub_seq_rows", C.c_int), ("eps", C.c_float)]


class VtLnBwd(C.Structure):
    _fields_ = [("dy", fp), ("xhat", fp), ("rstd", fp), ("gamma", fp), ("dpre", fp), ("dgamma", fp), ("dbeta", fp), ("M", C.c_long),
                ("accumulate", C.c_int), ("dy2", fp)]


class GlueMid(C.Structure):
    _fields_ = [("M", C.c_int), ("B", C.c_int), ("dxl", fp), ("dcs", fp), ("xhat", fp), ("rstd", fp), ("tn_w", fp * 5),
                ("g_tn_w", fp * 5), ("g_tn_b", fp * 5), ("dcond", fp), ("dea", fp), ("deb", fp), ("emb", fp), ("demb", fp)]


class AdamWEx(C.Structure):
    _fields_ = [("chunks", fp), ("n_chunks", C.c_int), ("params", fp), ("grads", fp), ("exp_avg", fp), ("exp_avg_sq", fp),
                ("ema", fp), ("step_lr", fp), ("lr", C.c_double), ("step", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("weight_decay", C.c_double), ("ema_decay", C.c_double), ("ema_warmup", C.c_int),
                ("grad_scale", fp)]


RESNET_FP32, RESNET_BF16 = 0, 1
IMG_F32_NCHW, IMG_U8_NHWC = 0, 1
RESNET50_NCONV = 53


class Conv(C.Structure):
    _fields_ = [("weight", fp), ("weight_bf16", fp), ("bias", fp), ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int),
                ("stride", C.c_int)]


class Resnet50(C.Structure):
    _fields_ = [("precision", C.c_int), ("conv", Conv * RESNET50_NCONV), ("tap", fp * 5)]


class RenderScene(C.Structure):
    _fields_ = [("verts", fp), ("faces", fp), ("points", fp), ("cams", fp)] + \
               [(n, C.c_int) for n in ("F", "NV", "NF", "P", "FC", "H", "W", "point_size")] + \
               [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "znear")]


class FlowHead(C.Structure):
    _fields_ = [(n, fp) for n in ("ctx_w", "ctx_b", "id_w", "lin_w", "bn_s", "bn_o", "res_b", "fin_w", "fin_b", "lu_w", "act_s",
                                  "act_o", "fc_w", "fc_b")] + [("id_parity", C.c_int), ("log_const", C.c_float)]


GEO_AA_TO_QUAT, GEO_AA_TO_ROTMAT, GEO_QUAT_TO_ROTMAT, GEO_ROT6D_PROHMR, GEO_ROT6D_DIFFUSION = range(5)

# name -> (restype, argtypes); every symbol of include/seeme_hip.h
_SIGNATURES = {
    "seeme_smpl_joints_backward": (C.c_int, [C.POINTER(SmplModel), fp, fp, fp, C.c_int, fp, fp, C.c_int, fp]),
    "seeme_smpl_joints_rot6d": (C.c_int, [C.POINTER(SmplModel), fp, fp, C.c_int, fp, C.c_int, fp, fp]),
    "seeme_smpl_joints_rot6d_backward": (C.c_int, [C.POINTER(SmplModel), fp, fp, C.c_int, fp, C.c_int, fp, fp, C.c_int, fp]),
    "seeme_vt_add_ln": (C.c_int, [C.POINTER(VtLn), fp]),
    "seeme_vt_ln_bwd": (C.c_int, [C.POINTER(VtLnBwd), fp]),
    "seeme_vt_softmax_fwd": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, fp]),
    "seeme_vt_softmax_bwd": (C.c_int, [fp, fp, C.c_long, C.c_int, C.c_float, fp]),
    "seeme_vt_gelu": (C.c_int, [fp, fp, fp, C.c_long, fp]),
    "seeme_vt_seq_sum": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, fp, C.c_float, fp]),
    "seeme_vt_dropout": (C.c_int, [fp, fp, C.c_float, fp, C.c_long, fp]),
    "seeme_vt_cross_rows": (C.c_int, [fp, fp, fp, fp, C.c_float, C.c_int, C.c_int, fp, fp]),
    "seeme_den_vecgrad": (C.c_int, [fp, C.c_int, C.c_int, fp, C.c_int, fp, C.c_int, fp, fp]),
    "seeme_glue_rows": (C.c_int, [C.POINTER(GlueRows), fp]),
    "seeme_glue_ln": (C.c_int, [fp, fp, fp, C.c_int, fp]),
    "seeme_glue_mid": (C.c_int, [C.POINTER(GlueMid), fp]),
    "seeme_grouped_gemm": (C.c_int, [fp, C.c_int, C.c_int, fp]),
    "seeme_gemm_problem_bytes": (C.c_int, []),
    "seeme_wgrad128": (C.c_int, [fp, C.c_long, fp, C.c_long, C.c_int, C.c_int, C.c_int, fp, C.c_long, fp, fp]),
    "seeme_gemm128": (C.c_int, [fp, C.c_long, fp, C.c_long, C.c_int, fp, C.c_long, C.c_int, C.c_int, C.c_int, fp, fp, C.c_long, fp]),
    "seeme_version": (C.c_int, []),
    "seeme_last_error": (C.c_char_p, []),
    "seeme_linear": (C.c_int, [C.POINTER(LinearArgs), fp]),
    "seeme_vae_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_vae_encode": (C.c_int, [C.POINTER(VaeWeights), fp, fp, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]),
    "seeme_vae_decode": (C.c_int, [C.POINTER(VaeWeights), fp, fp, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_vae_dec_prologue_bytes": (C.c_size_t, [C.c_int]),
    "seeme_vae_dec_prologue_h16": (C.c_int, [C.POINTER(VaeWeights), C.c_int, fp, C.c_size_t, fp]),
    "seeme_denoiser_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "seeme_denoiser_time_tables": (C.c_int, [C.POINTER(DenoiserWeights), fp, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_denoiser_cond_tables": (C.c_int, [C.POINTER(DenoiserWeights), fp, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_denoiser_ca_tables": (C.c_int, [C.POINTER(DenoiserWeights), fp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_denoiser_sample": (C.c_int, [C.POINTER(DenoiserWeights), C.POINTER(SampleArgs), fp]),
    "seeme_denoiser_tables1": (C.c_int, [C.POINTER(DenoiserWeights), fp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]),
    "seeme_denoiser_sample_cluster": (C.c_int, [C.POINTER(DenoiserWeights), C.POINTER(DenCluster), C.POINTER(SampleArgs), fp]),
    "seeme_den_cluster_xchg_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_den_cluster_ms_xchg_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "seeme_den_cluster_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "seeme_den_train_layout": (C.c_int, [C.POINTER(C.c_int64), C.c_int]),
    "seeme_den_train_pack": (C.c_int, [fp, fp, fp, fp, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_int, fp, fp]),
    "seeme_denoiser_backward": (C.c_int, [C.POINTER(DenoiserWeights), fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp]),
    "seeme_denoiser_backward_drop": (C.c_int, [C.POINTER(DenoiserWeights), fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_float, C.c_int, fp]),
    "seeme_den_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "seeme_den_wgrad": (C.c_int, [fp, C.c_int, C.c_int, fp, C.c_int, fp, fp]),
    "seeme_adamw_step": (C.c_int, [fp, C.c_int, fp, fp, fp, fp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                   C.c_double, fp]),
    "seeme_adamw_step_dev": (C.c_int, [fp, C.c_int, fp, fp, fp, fp, fp, C.c_double, C.c_double, C.c_double, C.c_double, fp]),
    "seeme_adamw_step_ex": (C.c_int, [C.POINTER(AdamWEx), fp]),
    "seeme_adamw_ex_bytes": (C.c_int, []),
    "seeme_grad_norm_workspace_bytes": (C.c_size_t, [C.c_int]),
    "seeme_grad_norm": (C.c_int, [fp, C.c_int, fp, C.c_double, fp, fp, C.c_size_t, fp]),
    "seeme_geometry": (C.c_int, [C.c_int, fp, fp, C.c_int, fp]),
    "seeme_renorm": (C.c_int, [fp, fp, fp, fp, C.c_long, C.c_int, fp]),
    "seeme_pointnet_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_pointnet_encode": (C.c_int, [C.POINTER(PointnetWeights), fp, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_pointnet_bf16_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_pointnet_encode_bf16": (C.c_int, [C.POINTER(PointnetWeights), C.POINTER(PointnetBf16), fp, C.c_int, C.c_int, fp, fp,
                                             C.c_size_t, fp]),
    "seeme_smpl_workspace_bytes": (C.c_size_t, [C.c_int]),
    "seeme_smpl_lbs": (C.c_int, [C.POINTER(SmplModel), fp, fp, C.c_int, fp, C.c_int, fp, fp, fp, C.c_size_t, fp]),
    "seeme_hyp_metrics_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "seeme_hyp_metrics": (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]),
    "seeme_hyp_pairdist_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "seeme_hyp_pairdist": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]),
    "seeme_social_metrics_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "seeme_social_metrics": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]),
    "seeme_overlap_cost_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "seeme_overlap_cost": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_path_select_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_path_select": (C.c_int, [fp, fp, C.c_int, C.c_int, fp, fp, fp, fp, C.c_size_t, fp]),
    "seeme_stitch_windows": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp]),
    "seeme_track_cost": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_float, fp, fp]),
    "seeme_track_filter": (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, fp, fp, fp]),
    "seeme_head_path_cost": (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp]),
    "seeme_head_anchor": (C.c_int, [fp, fp, C.c_int, C.POINTER(C.c_float), C.c_int, fp, fp, fp]),
    "seeme_head_rot_cost": (C.c_int, [fp, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, fp]),
    "seeme_scene_depth": (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                    C.c_int, fp, fp, fp, fp]),
    "seeme_scene_views_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "seeme_scene_views": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, C.c_size_t, fp]),
    "seeme_crop_patches": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, fp, fp]),
    "seeme_render_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "seeme_render": (C.c_int, [C.POINTER(RenderScene), fp, fp, fp, fp, C.c_size_t, fp]),
    "seeme_render_shade": (C.c_int, [C.POINTER(RenderScene), fp, fp, fp, C.c_int, fp, C.c_uint32, fp, fp]),
    "seeme_pa_mpjpe_frames": (C.c_int, [fp, fp, fp, C.c_int, fp, fp]),
    "seeme_mesh_v2v_frames": (C.c_int, [fp, fp, fp, fp, fp, C.c_int, C.c_int, fp, fp]),
    "seeme_scene_min_dist2_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "seeme_scene_min_dist2": (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_scene_inside_count_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "seeme_scene_inside_count": (C.c_int, [fp, fp, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_mesh_winding": (C.c_int, [fp, fp, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp]),
    "seeme_flow_head_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_flow_head": (C.c_int, [C.POINTER(FlowHead), fp, fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp, C.c_size_t, fp]),
    "seeme_resnet50_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "seeme_resnet50_encode": (C.c_int, [C.POINTER(Resnet50), fp, C.c_int, C.c_int, fp, fp, C.c_size_t, fp]),
    "seeme_resnet_conv": (C.c_int, [C.POINTER(Conv), C.c_int, fp, C.c_int, C.c_int, C.c_int, fp, C.c_int, fp, fp]),
    "seeme_resnet_stem_pack": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp]),
    "seeme_resnet_maxpool": (C.c_int, [C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and return the library; raises SeemeError when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SeemeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or seeme_amd/csrc/build.sh.  There is no CPU / PyTorch fallback for this path.")
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise SeemeError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(l, name)  # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().seeme_last_error().decode("utf-8", "replace")
        raise SeemeError(f"{what or 'seeme_hip'} failed (rc={rc}): {msg}")


def call(name: str, *args):
    """Invoke the status-returning entry point `name` with `args` as they are; a non-zero status raises SeemeError labelled `name`."""
    check(getattr(lib(), name)(*args), name)


class Workspace:
    """Grow-only scratch bytes for the launches that take a workspace.

    One uint8 buffer is held per key.  A request that fits gets the held tensor itself (all of it, not a slice); one that does not
    drops the held buffer first and then allocates, so the peak is the larger of the two and not their sum.

    The key is the device (`per_stream=False`), or the device plus the current stream's handle (`per_stream=True`; on a CPU device
    there is no stream and the key is the device alone).  A CUDA device without an index counts as the current one.  Buffers of
    other keys stay held: an object used on two devices keeps one buffer on each.  Both kinds exist for a reason:

    per_stream=False  the model objects (MldVae, MldDenoiser, ResnetPointnet, ResNet50, SMPL).  Their launches are warmed up on one
                      stream and captured on another (bench.py --graph; MLD.capture_training_step warms up on a side stream and
                      captures under torch.cuda.graph's own), so a buffer keyed by stream would be allocated for the first time
                      inside the capture.  One object's launches must therefore not overlap on two streams.
    per_stream=True   the module-level caches of the metric and recording functions, which any stream may call: launches of one
                      stream run in order, so they can share scratch, and launches of two streams never meet in one buffer.
    """

    def __init__(self, per_stream: bool):
        self.per_stream = per_stream
        self._held = {}

    def get(self, need: int, device):
        """uint8 tensor on `device` with numel() >= max(need, 16): the whole held buffer."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = device
        if self.per_stream and device.type == "cuda":
            key = (device, torch.cuda.current_stream(device).cuda_stream)
        ws = self._held.get(key)
        if ws is None or ws.numel() < max(need, 16):
            ws = None
            self._held.pop(key, None)
            ws = self._held[key] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=device)
        return ws

    def cached(self) -> list:
        """Every buffer currently held."""
        return list(self._held.values())

    def fill_(self, byte: int):
        """Overwrite every held buffer: no launch may depend on what an earlier one left (tests/test_gpu_vae_edges.py poisons it)."""
        for ws in self._held.values():
            ws.fill_(byte)


def default_xcds(chains: int, want="auto") -> int:
    """How many XCDs the working workgroups of a one-CU-per-chain launch sit on (SeemeSampleArgs.xcds): `want` = "auto" packs ~16
    chains per XCD -- right for a launch that has the chip to itself (one stream); callers that keep several launches in flight
    pass 8 (dealt over all XCDs).  SEEME_DEN_XCDS overrides (timing experiments, tests/test_gpu_flows.py)."""
    e = os.environ.get("SEEME_DEN_XCDS")
    if e is not None:
        want = int(e)
    if want == "auto":
        want = (chains + 15) // 16
    return min(8, max(1, int(want)))


def ptr(t) -> int:
    """Device pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_cuda(t, name: str):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SeemeError(f"{name} must be a tensor on the ROCm device (cuda:N); this path has no CPU fallback")
    if t.dtype != torch.float32:
        raise SeemeError(f"{name} must be float32, got {t.dtype}")
