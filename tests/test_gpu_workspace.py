"""The keying of seeme_amd._lib.Workspace on the device: a per-stream cache holds one buffer per stream, a per-object one holds one
buffer whatever the stream.  The model objects depend on the second kind: their launches are warmed up on one stream and captured
on another, and a buffer keyed by stream would be allocated inside the capture.  Needs a real MI355X: run with `pytest -m gpu`."""
import types

import pytest
import torch

from seeme_amd import _lib
from seeme_amd.weights_recipe import load_recipe_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def streams(dev):
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


def test_per_stream_workspace_holds_one_buffer_per_stream(dev, streams):
    s1, s2 = streams
    w = _lib.Workspace(per_stream=True)
    with torch.cuda.stream(s1):
        p1 = w.get(64, dev).data_ptr()
        assert w.get(64, dev).data_ptr() == p1
    with torch.cuda.stream(s2):
        p2 = w.get(64, dev).data_ptr()
    assert p2 != p1
    with torch.cuda.stream(s1):
        big = w.get(4096, dev)
        assert big.numel() >= 4096 and w.get(64, dev) is big
    with torch.cuda.stream(s2):
        assert w.get(64, dev).data_ptr() == p2
    assert len(w.cached()) == 2


def test_per_object_workspace_ignores_the_stream(dev, streams):
    s1, s2 = streams
    w = _lib.Workspace(per_stream=False)
    with torch.cuda.stream(s1):
        p = w.get(64, dev).data_ptr()
    with torch.cuda.stream(s2):
        assert w.get(64, dev).data_ptr() == p
    assert w.get(64, dev).data_ptr() == p
    with torch.cuda.device(dev):
        assert w.get(64, "cuda").data_ptr() == p          # no index: the current device, not a key of its own
    assert len(w.cached()) == 1


def test_vae_workspace_is_the_same_under_two_streams(dev, streams):
    """What bench.py --graph and MLD.capture_training_step rely on: the stream that captures finds the buffer of the stream that
    warmed up."""
    from seeme_amd.mld_vae import MldVae
    s1, s2 = streams
    abl = types.SimpleNamespace(MLP_DIST=False, PE_TYPE="mld", SKIP_CONNECT=True, VAE_TYPE="actor", DIFF_PE_TYPE="mld", MD_TRANS=True)
    vae = load_recipe_(MldVae(abl, nfeats=75, latent_dim=[1, 256], arch="encoder_decoder")).to(dev).eval()
    x = torch.randn(2, 8, 75, device=dev, generator=torch.Generator(dev).manual_seed(0))
    ptrs = [vae._workspace(2, 8, dev).data_ptr()]
    torch.cuda.synchronize(dev)
    out = []
    for s in (s1, s2):
        with torch.cuda.stream(s):
            out.append(vae.encode_dist(x, [8, 8]))
            ptrs.append(vae._workspace(2, 8, dev).data_ptr())       # under s: the buffer that launch was given
        s.synchronize()
        ptrs.append(vae._workspace(2, 8, dev).data_ptr())
    assert len(set(ptrs)) == 1 and len(ptrs) == 5
    assert len(vae._ws.cached()) == 1
    assert torch.equal(out[0], out[1])
