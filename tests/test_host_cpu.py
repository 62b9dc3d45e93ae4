"""CPU-side checks: the C-ABI library loads and exports every declared symbol, host logic
(schedulers, state-dict surface, packing layout) matches the oracle / the reference's key lists."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from oracle import mld_oracle as O
from seeme_amd import shapes


def _abl():
    return types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor",
                                 DIFF_PE_TYPE="mld", MD_TRANS=True)


def test_library_exports_every_declared_symbol():
    from seeme_amd import _lib
    lib = _lib.lib()   # raises if the .so is missing or a symbol is absent
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    declared = set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "header parse failed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/seeme_hip.h but not exported"
    assert declared <= set(_lib.exported_symbols()) | {"seeme_make_den_layout"}
    assert lib.seeme_version() >= 100


def test_signature_table_matches_every_header_prototype():
    """The whole ctypes table against the whole header: the same names, the same argument counts (a wrong argtypes length would
    first show up as a wild pointer on the GPU), and every name defined by the built library."""
    import subprocess
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    protos = re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", code)
    assert len(protos) >= 80, "header parse failed"
    names = [n for n, _ in protos]
    assert len(set(names)) == len(names)
    assert set(names) == set(re.findall(r"\b(seeme_[a-z_0-9]+)\s*\(", code)), "a prototype the parser could not read"
    for name, args in protos:
        assert name in _lib._SIGNATURES, f"{name} is declared in include/seeme_hip.h but has no ctypes signature"
        n = 0 if args.strip() in ("", "void") else args.count(",") + 1
        assert len(_lib._SIGNATURES[name][1]) == n, f"{name}: the header takes {n} arguments, argtypes has {len(_lib._SIGNATURES[name][1])}"
    assert set(_lib._SIGNATURES) <= set(names), f"not in the header: {sorted(set(_lib._SIGNATURES) - set(names))}"
    _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in nm.splitlines() if line.split()}
    assert set(names) <= defined, f"not defined by the library: {sorted(set(names) - defined)}"


def test_call_labels_a_failure_with_the_entry_point():
    from seeme_amd import _lib
    with pytest.raises(_lib.SeemeError) as e:      # F = 0: the argument check comes before any device work
        _lib.call("seeme_pa_mpjpe_frames", 16, 16, 16, 0, 16, 0)
    assert "seeme_pa_mpjpe_frames" in str(e.value) and "F must" in str(e.value)


_BAD_SAMPLE_ARGS = {
    "scheduler without coef": (dict(coef=None), "coefficient table"),
    "sched = 3": (dict(sched=3), "sched must be"),
    "steps = 0": (dict(steps=0), "steps must be >= 1"),
    "SCHED_NONE with two steps": (dict(sched=0, steps=2), "SCHED_NONE needs steps == 1"),
    "latents NULL": (dict(latents=None), "latents and out"),
    "out NULL": (dict(out=None), "latents and out"),
}


@pytest.mark.parametrize("entry", ["seeme_denoiser_sample", "seeme_denoiser_sample_cluster"])
@pytest.mark.parametrize("case", sorted(_BAD_SAMPLE_ARGS))
def test_sample_entry_points_share_one_argument_check(entry, case):
    """What both sampling entry points ask of SeemeSampleArgs is checked before anything else, by one function that labels the message
    with the entry point: a scheduler without its coefficient table, an unknown scheduler, no step, SCHED_NONE with more than one step,
    no latents, no output.  Weights and cluster are all-zero structs and the table pointers address one host float that nothing may read,
    so a case that got past the shared check would fail on the per-entry ones with another message -- never reach a launch."""
    from seeme_amd import _lib
    lib = _lib.lib()
    host = (C.c_float * 1)()
    p = C.addressof(host)
    a = _lib.SampleArgs()
    a.B, a.N, a.steps, a.sched, a.guidance_scale = 2, 1, 2, _lib.SCHED_DDIM, 1.0
    a.latents, a.ctab, a.ttab, a.trow, a.coef, a.out = p, p, p, p, p, p
    fields, what = _BAD_SAMPLE_ARGS[case]
    for k, v in fields.items():
        setattr(a, k, v)
    w, cl = _lib.DenoiserWeights(), _lib.DenCluster()
    args = (C.byref(w), C.byref(a), None) if entry == "seeme_denoiser_sample" else (C.byref(w), C.byref(cl), C.byref(a), None)
    assert getattr(lib, entry)(*args) != 0
    msg = lib.seeme_last_error().decode()
    assert msg.startswith(entry[len("seeme_"):] + ": ") and what in msg, msg
    with pytest.raises(_lib.SeemeError, match=entry):
        _lib.call(entry, *args)


def test_workspace_grows_only_and_holds_one_buffer_per_key():
    from seeme_amd import _lib
    cpu = torch.device("cpu")
    w = _lib.Workspace(per_stream=False)
    a = w.get(100, cpu)
    assert a.dtype == torch.uint8 and a.numel() >= 100
    assert w.get(50, cpu) is a
    b = w.get(200, cpu)
    assert b is not a and b.numel() >= 200
    assert len(w.cached()) == 1 and w.cached()[0] is b
    assert w.get(0, cpu) is b
    w.fill_(0xA5)
    assert bool((b == 0xA5).all())
    assert _lib.Workspace(per_stream=False).get(0, cpu).numel() >= 16
    assert _lib.Workspace(per_stream=True).get(0, cpu).numel() >= 16          # no stream on the CPU: keyed by the device alone


def test_pointnet_bf16_struct_mirrors_header():
    """SeemePointnetBf16 holds nothing but pointers, so member names, order and array lengths are its whole layout: the
    ctypes mirror has to repeat the header exactly (a mismatch would first show up as a wild pointer on the GPU)."""
    from seeme_amd import _lib
    hdr = open(os.path.join(REPO, "include", "seeme_hip.h")).read()
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*SeemePointnetBf16;", hdr, re.S)
    assert m, "SeemePointnetBf16 not found in include/seeme_hip.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    members = []
    for d in decls:
        mm = re.fullmatch(r"const\s+(?:uint16_t|float)\s*\*\s*(\w+)(?:\[(\d+)\])?", d)
        assert mm, f"unexpected member declaration: {d!r}"
        members.append((mm.group(1), int(mm.group(2)) if mm.group(2) else None))
    assert members == [("posf", None), ("stream", 4), ("sc3f", None)]
    mirror = [(name, ctype._length_ if issubclass(ctype, C.Array) else None) for name, ctype in _lib.PointnetBf16._fields_]
    assert mirror == members
    for _, ctype in _lib.PointnetBf16._fields_:
        assert (ctype._type_ if issubclass(ctype, C.Array) else ctype) is C.c_void_p
    assert C.sizeof(_lib.PointnetBf16) == 6 * C.sizeof(C.c_void_p)


def test_den_layout_is_consistent():
    from seeme_amd import _lib
    n = 155
    buf = (C.c_int64 * n)()
    assert _lib.lib().seeme_den_layout(1024, 128, buf, n) == 0
    v = list(buf)
    wg_total, vp_total = v[153], v[154]
    # matrices of one step: 5 layers + 2 skip linears
    per_layer = 3 * 65536 + 65536 + 2 * 1024 * 256 + 2 * 65536 + 2 * 128 * 256 + 65536
    assert wg_total == 5 * per_layer + 2 * 2 * 65536
    assert vp_total > 0 and v[0] == -1 and v[3 * 30] >= 0   # skip offset only for layers 3,4


def test_no_cpu_fallback():
    from seeme_amd.mld_vae import MldVae
    from seeme_amd._lib import SeemeError
    vae = MldVae(_abl(), nfeats=75, arch="encoder_decoder")
    with pytest.raises(SeemeError):
        vae.encode(torch.zeros(1, 8, 75), None, [8])


def test_state_dict_surface_matches_reference_key_lists():
    from seeme_amd.mld_vae import MldVae
    from seeme_amd.mld_denoiser import MldDenoiser
    vae = MldVae(_abl(), nfeats=75, arch="encoder_decoder")
    sd = {k: tuple(v.shape) for k, v in vae.state_dict().items()}
    assert sd == shapes.vae_shapes(75)
    assert sum(int(np.prod(s)) for s in sd.values()) == 5441099
    den = MldDenoiser(_abl(), condition=["text", "interactee"], ff_size=128, num_layers=5, num_heads=1)
    sd = {k: tuple(v.shape) for k, v in den.state_dict().items()}
    assert sd == shapes.denoiser_shapes()
    assert sum(int(np.prod(s)) for s in sd.values()) == 7900032


def test_unsupported_configs_raise_like_the_reference():
    from seeme_amd.mld_vae import MldVae
    from seeme_amd.mld_denoiser import MldDenoiser
    a = _abl()
    a.PE_TYPE = "bogus"
    with pytest.raises(ValueError):
        MldVae(a, nfeats=75, arch="encoder_decoder")
    with pytest.raises(ValueError):
        MldVae(_abl(), nfeats=75, arch="bogus")
    with pytest.raises(ValueError):
        MldDenoiser(_abl(), condition=["text"], arch="bogus", num_layers=5, num_heads=1)
    with pytest.raises(TypeError):
        MldDenoiser(_abl(), condition=["scene"], num_layers=5, num_heads=1)


def test_schedulers_match_oracle():
    from seeme_amd.schedulers import DDIMScheduler, DDPMScheduler
    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
    ddim = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, **kw)
    ddim.set_timesteps(50)
    acp = O.alphas_cumprod(O.make_betas())
    assert np.allclose(ddim.alphas_cumprod.numpy(), acp, rtol=1e-6)
    assert ddim.timesteps.tolist() == O.ddim_timesteps(50).tolist()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 1, 256)).astype(np.float32)
    e = rng.standard_normal((3, 1, 256)).astype(np.float32)
    n = rng.standard_normal((3, 1, 256)).astype(np.float32)
    for t in (981, 501, 1):
        for eta in (0.0, 0.5):
            got = ddim.step(torch.from_numpy(e), t, torch.from_numpy(x), eta=eta, variance_noise=torch.from_numpy(n)).prev_sample
            assert rel_err(got.numpy(), O.ddim_step(acp, e, t, x, 50, eta, n)) < 1e-5
    # the coefficient table reproduces step() (this is what the fused kernel consumes)
    c = ddim.coef_table(0.5).numpy()
    for i, t in enumerate(ddim.timesteps.tolist()[:3]):
        x0 = (x - c[i, 1] * e) / c[i, 0]
        prev = c[i, 2] * x0 + c[i, 3] * e + c[i, 5] * x + c[i, 4] * n
        assert rel_err(prev, O.ddim_step(acp, e, t, x, 50, 0.5, n)) < 1e-5
    ddpm = DDPMScheduler(variance_type="fixed_small", **kw)
    tt = np.array([999, 0, 37])
    got = ddpm.add_noise(torch.from_numpy(x), torch.from_numpy(n), torch.from_numpy(tt))
    assert rel_err(got.numpy(), O.ddpm_add_noise(acp, x, n, tt)) < 1e-6
    ddpm.set_timesteps(1000)
    for t in (999, 500, 0):
        got = ddpm.step(torch.from_numpy(e), t, torch.from_numpy(x), variance_noise=torch.from_numpy(n)).prev_sample
        assert rel_err(got.numpy(), O.ddpm_step(acp, e, t, x, n)) < 1e-5
    c = ddpm.coef_table().numpy()
    i = 0
    x0 = (x - c[i, 1] * e) / c[i, 0]
    assert rel_err(c[i, 2] * x0 + c[i, 5] * x + c[i, 4] * n, O.ddpm_step(acp, e, 999, x, n)) < 1e-5


def test_timestep_features_match_oracle():
    from seeme_amd.mld_denoiser import timestep_features
    t = torch.tensor([0, 1, 21, 501, 981, 999])
    assert rel_err(timestep_features(t).numpy(), O.timestep_features(t.numpy())) < 1e-4


def test_config_loader_own_and_reference_yaml(tmp_path):
    import yaml
    from seeme_amd.config import TARGET_MAP, parse_config, instantiate_from_config
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_scene.yaml"))
    assert cfg.model.condition == ["text", "scene", "interactee"]
    assert cfg.model.denoiser.params.ablation.MD_TRANS is True
    assert cfg.model.denoiser.params.latent_dim == [1, 256]
    assert isinstance(cfg.TRAIN.OPTIM.LR, float)
    den = instantiate_from_config(cfg.model.denoiser)
    sch = instantiate_from_config(cfg.model.scheduler)
    assert type(den).__name__ == "MldDenoiser" and type(sch).__name__ == "DDIMScheduler"
    # the same tree in the reference's layout, every module `target` spelled with the reference's class path
    ref_target = {v: k for k, v in TARGET_MAP.items()}
    for fn in ("base.yaml", "config_mld_egobody.yaml"):
        (tmp_path / fn).write_text(open(os.path.join(REPO, "configs", fn)).read())
    os.makedirs(tmp_path / "modules")
    for fn in os.listdir(os.path.join(REPO, "configs", "modules")):
        node = yaml.safe_load(open(os.path.join(REPO, "configs", "modules", fn)))
        for v in node.values():
            if isinstance(v, dict) and v.get("target") in ref_target:
                v["target"] = ref_target[v["target"]]
        (tmp_path / "modules" / fn).write_text(yaml.safe_dump(node))
    # loader semantics the layout relies on: an assets.yaml merged last, a module whose target this package does not
    # provide, and references to keys no file defines -- resolved lazily by OmegaConf, so kept as written here
    (tmp_path / "assets.yaml").write_text("FOLDER: ./runs\nmodel:\n  asset_path: ./deps/asset\n")
    (tmp_path / "modules" / "zz_unmapped.yaml").write_text(
        "probe:\n  target: pkg.unmapped.Probe\n  params:\n    path: ${model.asset_path}\n    size: ${model.undefined_node.size}\n"
        "    label: size ${model.undefined_node.size} of ${model.nfeats}\n")
    r = parse_config(str(tmp_path / "config_mld_egobody.yaml"))
    assert r.FOLDER == "./runs" and r.model.asset_path == "./deps/asset"
    assert r.model.probe.target == "pkg.unmapped.Probe" and r.model.probe.params.path == "./deps/asset"
    assert r.model.probe.params.size == "${model.undefined_node.size}"
    assert r.model.probe.params.label == "size ${model.undefined_node.size} of ${model.nfeats}"
    assert r.model.denoiser.target == "mld.models.architectures.mld_denoiser.MldDenoiser"   # kept as written
    assert r.model.motion_vae.target == "mld.models.architectures.mld_vae.MldVae"
    assert r.model.scheduler.target == "diffusers.DDIMScheduler"
    assert type(instantiate_from_config(r.model.denoiser)).__module__ == "seeme_amd.mld_denoiser"
    assert type(instantiate_from_config(r.model.motion_vae)).__module__ == "seeme_amd.mld_vae"
    assert type(instantiate_from_config(r.model.scheduler)).__module__ == "seeme_amd.schedulers"
    assert r.model.scheduler.num_inference_timesteps == 50


def test_mld_constructs_from_config_on_cpu():
    from seeme_amd.config import parse_config
    from seeme_amd.mld import MLD, SyntheticEgoDataModule
    from seeme_amd.smpl import SMPL
    cfg = parse_config(os.path.join(REPO, "configs", "config_mld_scene.yaml"))
    m = MLD(cfg, SyntheticEgoDataModule(), smpl_model=SMPL.synthetic(1, V=64))
    keys = set(m.state_dict().keys())
    assert "vae.encoder.input_blocks.0.self_attn.in_proj_weight" in keys
    assert "denoiser.encoder.middle_block.sa_block.linear1.weight" in keys
    assert "proscene.scene_enc.block_3.shortcut.weight" in keys and "output_scene.1.weight" in keys
    assert "smpl_model.lbs_weights" in keys
    for name in ("training_step", "validation_step", "test_step", "allsplit_step", "_diffusion_reverse",
                 "_diffusion_process", "train_vae_forward", "train_diffusion_forward", "ego_eval", "configure_optimizers"):
        assert callable(getattr(m, name))


# ----------------------------------------------------------------------------- CLI plumbing (no GPU work)
def test_cli_arguments_and_experiment_folder(tmp_path):
    from seeme_amd import cli
    args = cli.build_parser("train").parse_args(["--cfg", os.path.join(REPO, "configs", "config_mld_egobody.yaml"),
                                                 "--batch_size", "8", "--nodebug", "--folder", str(tmp_path)])
    cfg = cli.load_cfg(args, "train")
    assert cfg.TRAIN.BATCH_SIZE == 8 and cfg.DEBUG is False
    assert cfg.FOLDER_EXP == os.path.join(str(tmp_path), "mld", "s2_interactee")
    with pytest.raises(NotImplementedError):
        cli.load_cfg(cli.build_parser("test").parse_args(["--cfg", args.cfg, "--dir", "x"]), "test")


def test_cli_checkpoint_layout_roundtrip(tmp_path):
    """Lightning layout ({"state_dict": ...}, epoch=<n>.ckpt), newest-epoch resume scan, strict vae.* sub-load."""
    import torch
    from seeme_amd import cli

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vae = torch.nn.Linear(3, 2)
            self.denoiser = torch.nn.Linear(2, 2)
            self.optimizer = None

    m = Tiny()
    m.optimizer = torch.optim.AdamW(m.parameters(), lr=1e-3)
    d = tmp_path / "exp"
    for e in (0, 2, 10):
        cli.save_checkpoint(str(d / "checkpoints" / f"epoch={e}.ckpt"), m, e, 8 * (e + 1))
    newest = cli.newest_checkpoint(str(d))
    assert newest.endswith("epoch=10.ckpt")                       # numeric, not lexicographic, order
    ck = cli.read_checkpoint(newest)
    assert set(ck["state_dict"]) == set(m.state_dict()) and ck["epoch"] == 10 and ck["global_step"] == 88
    m2 = Tiny()
    assert cli.load_pretrained_vae(m2, newest) == 2
    assert torch.equal(m2.vae.weight, m.vae.weight) and not torch.equal(m2.denoiser.weight, m.denoiser.weight)
    with pytest.raises(ValueError):
        cli.newest_checkpoint(str(tmp_path / "missing"))


# ----------------------------------------------------------------------------- device-side ComputeMetrics
@pytest.mark.parametrize("split", ["test", "val"])
def test_ego_metrics_match_reference_loops(split):
    """Vectorised, device-resident metrics vs the oracle's restatement of the reference's per-sequence numpy loops
    (metrics/compute.py:349-580): ragged lengths, sequences excluded by the test-split rule, a static sequence."""
    from seeme_amd.mld import EgoMetrics
    rng = np.random.default_rng(5)
    B, T = 6, 20
    ref = rng.standard_normal((B, T, 24, 3)) * 0.3
    pred = ref + rng.standard_normal((B, T, 24, 3)) * np.array([0.02, 0.05, 0.02, 0.6, 0.02, 0.02])[:, None, None, None]
    pred[4] = ref[4]                  # identical: zero acceleration error -> never counted (compute.py:503,567)
    qg = rng.standard_normal((B * T, 4))
    qg /= np.linalg.norm(qg, axis=1, keepdims=True)
    dq = np.concatenate([np.ones((B * T, 1)), 0.05 * rng.standard_normal((B * T, 3))], axis=1)
    dq[T:2 * T, 1:] *= 30             # sequence 1: large head-orientation error -> excluded on 'test'
    qp = qg + 0.0
    qp = np.stack([qg[:, 0] * dq[:, 0] - (qg[:, 1:] * dq[:, 1:]).sum(1),
                   qg[:, 0] * dq[:, 1] + dq[:, 0] * qg[:, 1] + qg[:, 2] * dq[:, 3] - qg[:, 3] * dq[:, 2],
                   qg[:, 0] * dq[:, 2] + dq[:, 0] * qg[:, 2] + qg[:, 3] * dq[:, 1] - qg[:, 1] * dq[:, 3],
                   qg[:, 0] * dq[:, 3] + dq[:, 0] * qg[:, 3] + qg[:, 1] * dq[:, 2] - qg[:, 2] * dq[:, 1]], axis=1)
    lengths = [20, 20, 13, 20, 20, 7]
    want = O.ego_metrics(pred, ref, qp, qg, lengths, split)
    m = EgoMetrics()
    half = 3
    for sl in (slice(0, half), slice(half, B)):       # two updates, as over two batches
        m.update(torch.from_numpy(pred[sl]).float(), torch.from_numpy(ref[sl]).float(), lengths[sl],
                 torch.from_numpy(qp.reshape(B, T, 4)[sl].reshape(-1, 4)).float(),
                 torch.from_numpy(qg.reshape(B, T, 4)[sl].reshape(-1, 4)).float(), split=split)
    got = m.compute()
    assert got["count_seq"] == want["count_seq"] and 0 < got["count_seq"] < B
    for k in ("MPJPE", "ROOT_ERROR", "ACCL", "HEAD_ORIENTATION_ERROR"):
        assert abs(got[k] - want[k]) <= 2e-4 * max(1.0, abs(want[k])), (k, got[k], want[k])


# ----------------------------------------------------------------------------- SMPL model files
def test_smpl_pkl_loader_is_code_free(tmp_path):
    """A user-supplied SMPL_*.pkl is read with an allow-listing unpickler: arrays and sparse matrices load, any other
    global (the way a pickle executes code) is refused."""
    import pickle
    import scipy.sparse as sp
    from seeme_amd import smpl as S
    V = 40
    rng = np.random.default_rng(0)
    d = {"v_template": rng.standard_normal((V, 3)), "shapedirs": rng.standard_normal((V, 3, 10)),
         "posedirs": rng.standard_normal((V, 3, 207)), "J_regressor": sp.csc_matrix(rng.random((24, V))),
         "weights": rng.random((V, 24)), "kintree_table": np.stack([np.array(S.SMPL_PARENTS, np.int64) % (2 ** 32), np.arange(24)]),
         "f": np.zeros((5, 3), np.uint32)}
    good = tmp_path / "SMPL_NEUTRAL.pkl"
    good.write_bytes(pickle.dumps(d, protocol=2))
    out = S._load_model_file(str(tmp_path))
    assert out["J_regressor"].shape == (24, V) and out["posedirs"].shape == (207, V * 3) and out["parents"][0] == -1
    np.testing.assert_allclose(out["v_template"], d["v_template"].astype(np.float32))

    class Evil:
        def __reduce__(self):
            import os
            return (os.system, ("echo pwned > " + str(tmp_path / "pwned"),))

    bad = tmp_path / "bad.pkl"
    bad.write_bytes(pickle.dumps({"v_template": Evil()}, protocol=2))
    with pytest.raises(pickle.UnpicklingError):
        S._load_model_file(str(bad))
    assert not (tmp_path / "pwned").exists()


# ----------------------------------------------------------------------------- PointNet v2: packing of the weight streams
def test_pointnet_v2_stream_packing_emulated():
    """The PointNet block kernels (csrc/pointnet_bf16.hip) consume host-packed weight streams whose k order
    encodes the kernel's register layouts (accumulator tile pair -> next B operand), and keep the activations between
    blocks in that fragment order.  This emulates the kernel's dataflow on the CPU -- MFMA semantics on the packed
    fragments, slot by slot, bf16 rounding where the kernel rounds, the activation layout of the stores / loads -- and
    compares with the oracle's PointNet: a wrong permutation is an O(1) error."""
    from oracle import mld_oracle as O
    from seeme_amd import shapes
    from seeme_amd.respointnet import ResnetPointnet
    from seeme_amd.weights_recipe import load_recipe_, recipe_state_dict
    pn = load_recipe_(ResnetPointnet(512, 256)).eval()
    bf = [getattr(pn, f"block_{i}") for i in range(4)]
    ws0 = bf[0].shortcut.weight.double()
    sc3 = torch.cat([ws0 @ pn.fc_pos_0.weight.double(), (ws0 @ pn.fc_pos_0.bias.double())[:, None]], dim=1).float()
    with torch.no_grad():
        streams, sc3f = pn._pack_streams(bf, sc3)
    assert all(s.shape == (24, 16, 64, 8) for s in streams) and sc3f.shape == (16, 4, 16, 4)
    bf16 = lambda t: t.to(torch.bfloat16).float()

    def mfma(A, Bf):          # A, Bf: [64 lanes, 8]; lane = 16 kq + (row | col) -> D[row m][col r]
        return torch.einsum("qmj,qrj->mr", A.float().view(4, 16, 8), Bf.float().view(4, 16, 8))

    rng = np.random.default_rng(11)
    P = 40                                        # one scene, 40 points = 3 point tiles (the last one ragged)
    NT = (P + 15) // 16
    pts = torch.from_numpy(rng.uniform(-3, 3, (P, 3)).astype(np.float32))
    kq, r = torch.arange(64) // 16, torch.arange(64) % 16
    jj = torch.arange(8)[None]
    pad = lambda x, n: torch.cat([x, torch.zeros(n - x.shape[0], *x.shape[1:])])

    def acc_pair_to_frag(acc, kb):                # accumulator tiles (2 kb, 2 kb + 1) [tile][row m][col r] -> B fragment [64 lanes, 8]
        return acc[2 * kb + jj // 4, 4 * kq[:, None] + jj % 4, r[:, None]]

    def run_block(i, xin, v0, vs):
        """xin: block_0 -> points [P,3]; later -> activations in fragment order [NT][8 kb][64 lanes][8] (bf16 values).
        Returns (activations in fragment order, per-feature max over the valid points)."""
        b0 = bf[i].fc_0.bias.detach() + (v0 if v0 is not None else 0)
        b1 = bf[i].fc_1.bias.detach() + (vs if vs is not None else 0)
        st = streams[i].float()
        out = torch.zeros(NT, 8, 64, 8)
        pool = torch.full((256,), -float("inf"))
        nk0 = 16 if i == 0 else 8
        m_idx = torch.arange(16)
        for pt in range(NT):                      # one 16-point tile (mt) at a time
            p0 = pt * 16
            acc0 = (b0.view(16, 16)[:, :, None]).expand(16, 16, 16).clone()          # accumulator starts at the bias: [nt][row m][col r]
            if i == 0:
                x512 = bf16(torch.relu(pad(pts[p0:p0 + 16], 16) @ pn.fc_pos_0.weight.T + pn.fc_pos_0.bias)).T      # [feature][point]
            for s in range(nk0):
                if i == 0:                        # generated input: small-MFMA tiles (2 s, 2 s + 1) -> B fragment
                    Bf = acc_pair_to_frag(x512.view(32, 16, 16), s)
                else:
                    Bf = torch.relu(xin[pt, s])
                for nt in range(16):
                    acc0[nt] += mfma(st[s, nt], Bf)
            hf = [bf16(torch.relu(acc_pair_to_frag(acc0, kb))) for kb in range(8)]
            for g in range(2):
                acc1 = (b1.view(16, 16)[8 * g:8 * g + 8, :, None]).expand(8, 16, 16).clone()
                base = nk0 + (4 if i == 0 else 8) * g
                if i == 0:                        # slot base + p: fc_1 k-blocks 2p, 2p + 1 (fragments 8 kbi + n)
                    for p in range(4):
                        for kbi in range(2):
                            for n in range(8):
                                acc1[n] += mfma(st[base + p, kbi * 8 + n], hf[2 * p + kbi])
                    fr = sc3f.float().permute(0, 2, 1, 3)             # [n-tile][m][kq][4]
                    px, py, pz = (pad(pts[p0:p0 + 16], 16)[:, c] for c in range(3))
                    h = lambda v: bf16(v)
                    l = lambda v: bf16(v - bf16(v))
                    one = torch.ones(16)
                    kslots = torch.stack([torch.stack([h(px), h(py), h(pz), l(px)], -1), torch.stack([l(py), l(pz), h(px), h(py)], -1),
                                          torch.stack([h(pz), one, one, 0 * one], -1), torch.zeros(16, 4)], dim=1)       # [point][kq][4]
                    for n in range(8):
                        acc1[n] += torch.einsum("mqj,rqj->mr", fr[8 * g + n], kslots)
                else:                             # slot base + kb: shortcut k-block kb (fragments 0..7, raw x) | fc_1 k-block kb (8..15, hidden)
                    for kb in range(8):
                        for n in range(8):
                            acc1[n] += mfma(st[base + kb, n], xin[pt, kb]) + mfma(st[base + kb, 8 + n], hf[kb])
                for kl in range(4):               # the stored fragment of k-block 4 g + kl = tiles (2 kl, 2 kl + 1) of this half
                    out[pt, 4 * g + kl] = bf16(acc_pair_to_frag(acc1, kl))
                valid = min(16, P - p0)
                mx = bf16(acc1[:, :, :valid]).max(dim=2).values                      # [tile n][row m] -> feature 16 (8 g + n) + m
                pool[128 * g:128 * g + 128] = torch.maximum(pool[128 * g:128 * g + 128], mx.reshape(-1))
        return out, pool

    with torch.no_grad():
        act, pooled = run_block(0, pts, None, None)
        for i in (1, 2, 3):
            W0, Ws = bf[i].fc_0.weight.detach(), bf[i].shortcut.weight.detach()
            act, pooled_new = run_block(i, act, W0[:, 256:] @ torch.relu(pooled), Ws[:, 256:] @ pooled)
            pooled = pooled_new
        got = (pn.fc_c.weight @ torch.relu(pooled) + pn.fc_c.bias).numpy()
    want = O.pointnet_forward(recipe_state_dict(shapes.pointnet_shapes()), pts.numpy()[None])[0]
    assert rel_err(got, want) < 3e-2, rel_err(got, want)


def test_grouped_gemm_descriptor_layout_and_tiling():
    """The ctypes mirror of SeemeGemmProblem has the library's size (the descriptor tables are byte images built on the host),
    and _Group lays the 64 x 64 tiles of its problems out back to back, batched members included."""
    import ctypes as C
    from seeme_amd import _lib as L
    from seeme_amd.stage2_glue import _prob, _tiles
    assert C.sizeof(L.GemmProblem) == L.lib().seeme_gemm_problem_bytes()
    assert _tiles(64, 64) == (1, 1) and _tiles(65, 130) == (6, 3) and _tiles(198, 198) == (16, 4)
    p = _prob([1000], [2000], [256], [1], [1], 256, 256, 3000, 768, 198, 768, bias=4000)
    q = _prob([1000], [2000], [198], [198], [256], 1, 1, 5000, 768, 198, 256, nbatch=7, bstrides=(198 * 198, 198 * 256, 198 * 768),
              accumulate=2, colsum=6000)
    assert (p.nseg, p.seg_len[0], p.a_rs, p.b_cs, p.ldc, p.M, p.N, p.nbatch) == (1, 256, 256, 256, 768, 198, 768, 1)
    assert (q.a_ks[0], q.b_ks[0], q.accumulate, q.nbatch, q.a_bstride, q.c_bstride) == (198, 256, 2, 7, 198 * 198, 198 * 768)
    t0 = 0
    for pr in (p, q):                                      # what _Group does before it uploads the table
        n, tn = _tiles(pr.M, pr.N)
        pr.tile0, pr.tiles_n = t0, tn
        t0 += n * max(1, pr.nbatch)
    assert (p.tile0, p.tiles_n, q.tile0, q.tiles_n, t0) == (0, 12, 48, 4, 48 + 16 * 7)


def test_cluster_weight_image_indexing():
    """seeme_amd.mld_denoiser.cluster_pack_stage against the indexing k_den_cluster applies (csrc/den_cluster.inc.hip: cl_issue /
    cl_consume): wave w, unit u, load i of the unit -> stage load j = u UL + i -> k-block j // TPW, tile w TPW + j % TPW; lane
    16 g + r, element e -> W[16 tile + r][KL kb + (KL / 4) g + e].  Both element widths, every tiles-per-wave count in use."""
    import torch
    from seeme_amd.mld_denoiser import cluster_pack_stage
    g = torch.Generator().manual_seed(3)
    for KL, UL in ((32, 8), (16, 16)):
        for TPW, K in ((1, 256), (1, 512), (2, 128), (2, 256), (4, 256), (2, 512)):
            W = torch.randn(8 * TPW * 16, K, generator=g)
            img = cluster_pack_stage(W, TPW, KL, UL)
            units = (K // KL) * TPW // UL
            assert tuple(img.shape) == (units, 8, UL, 64, KL // 4)
            for (u, w, i, lane, e) in [(0, 0, 0, 0, 0), (units - 1, 7, UL - 1, 63, KL // 4 - 1), (units // 2, 3, 5, 37, 2), (0, 6, 1, 16, 1)]:
                j = u * UL + i
                kb, t = j // TPW, j % TPW
                row, col = 16 * (w * TPW + t) + (lane & 15), KL * kb + (KL // 4) * (lane >> 4) + e
                assert img[u, w, i, lane, e] == W[row, col]
            # every element appears exactly once
            assert torch.equal(torch.sort(img.reshape(-1))[0], torch.sort(W.reshape(-1))[0])


def test_bench_dump_outputs_float32_and_seeded_sample_over_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: every array as <name>.npy in float32; one over the byte budget is cut to a fixed, seeded,
    sorted sample of its rows, whose indices land in <name>_rows.npy."""
    import bench
    x = torch.arange(10 * 6, dtype=torch.float16).reshape(10, 2, 3)
    bench.dump_outputs(str(tmp_path / "a"), {"feats": x})
    a = np.load(tmp_path / "a" / "feats.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.float().numpy())
    assert sorted(os.listdir(tmp_path / "a")) == ["feats.npy"]
    monkeypatch.setattr(bench, "DUMP_BYTES", 100)          # 24 bytes per row + 8 per index: 3 of the 10 rows
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"feats": x})
    rows = np.load(tmp_path / "b" / "feats_rows.npy")
    b = np.load(tmp_path / "b" / "feats.npy")
    assert rows.dtype == np.float64 and len(rows) == 3 and np.all(np.diff(rows) > 0)
    assert b.dtype == np.float32 and np.array_equal(b, x.float().numpy()[rows.astype(np.int64)])
    assert b.nbytes + rows.nbytes <= 100
    assert np.array_equal(rows, np.load(tmp_path / "c" / "feats_rows.npy"))
    assert np.array_equal(b, np.load(tmp_path / "c" / "feats.npy"))
    # smallest first: the scalar is written whole, the rest of the budget goes to the large array
    bench.dump_outputs(str(tmp_path / "d"), {"feats": x, "loss": torch.tensor(2.5)})
    assert np.load(tmp_path / "d" / "loss.npy") == np.float32(2.5)
    assert len(np.load(tmp_path / "d" / "feats_rows.npy")) == 3       # 96 bytes left: 3 rows of 24 + 3 indices
    # one row alone over the budget: a seeded sample of the flattened elements
    monkeypatch.setattr(bench, "DUMP_BYTES", 30)                      # a row needs 24 + 8; an element 4 + 8: 2 elements
    bench.dump_outputs(str(tmp_path / "e"), {"feats": x})
    rows = np.load(tmp_path / "e" / "feats_rows.npy")
    e = np.load(tmp_path / "e" / "feats.npy")
    assert e.shape == (2,) and np.array_equal(e, x.float().numpy().reshape(-1)[rows.astype(np.int64)])
    monkeypatch.setattr(bench, "DUMP_BYTES", 8)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "f"), {"feats": x})
