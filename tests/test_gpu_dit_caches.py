"""GPU suite: the eviction of the DiT forward's time and group tables (csrc/dit.hip: cache_slot under time_entry / group_tables).

Host bookkeeping is under test, so the model is tiny: f32, D = 32, two layers, 3 x 4 x 6 = 72 tokens, 8 text tokens (the kernels'
own shapes are held by test_gpu_dit_frames.py, test_gpu_normfold.py and the model suites).  One handle sees more distinct
timestep vectors (per-frame matrices) than its cache has entries, so the first ones are evicted and their slots overwritten; the
forwards that come back to an evicted and to a still cached key must return, bit for bit, what a fresh handle returns there."""
import pytest
import torch

import ltx_oracle as O
from tools_cfg import PIPE_DIT_CFG

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(PIPE_DIT_CFG, num_layers=2)
F, H, W, K = 3, 4, 6, 8
TIME_ENTRIES, GROUP_ENTRIES = 64, 8      # kDitTimeEntries, kDitGroupEntries (csrc/dit.hip)


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


@pytest.fixture(scope="module")
def fresh(hip):
    w = {k: v.to(DEV) for k, v in O.synth_weights(O.dit_weight_shapes(O.DitConfig(**CFG)), seed=91).items()}
    return lambda: hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**CFG), w, torch.float32)


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(92)
    hidden = torch.randn(1, F * H * W, CFG["in_channels"], generator=g); enc = torch.randn(1, K, CFG["caption_channels"], generator=g)
    mask = torch.ones(1, K); mask[:, 5:] = 0
    return hidden.to(DEV), enc.to(DEV), mask.to(DEV), O.build_video_coords(1, F, H, W).to(DEV)


def forward(m, inputs, t, frames=False):
    hidden, enc, mask, coords = inputs
    y = (m.forward_frames if frames else m.forward)(hidden, enc, t, mask, F, H, W, None, coords, None)
    torch.cuda.synchronize()
    return y.cpu()


def test_time_tables_survive_eviction(fresh, inputs):
    ts = [torch.tensor([float(3 + 7 * i)]) for i in range(TIME_ENTRIES + 2)]
    used = fresh()
    first_pass = [forward(used, inputs, t) for t in ts]
    for i in (0, len(ts) - 1):                              # the first key was evicted two misses ago, the last one is still cached
        want = forward(fresh(), inputs, ts[i])
        assert torch.isfinite(want).all() and not torch.equal(want, first_pass[i - 1])      # (the timestep does move the output)
        assert torch.equal(first_pass[i], want), i
        assert torch.equal(forward(used, inputs, ts[i]), want), i


def test_group_tables_survive_eviction(fresh, inputs):
    ts = [torch.tensor([[float(5 + 11 * j), float(400 + 13 * j), 0.0]]) for j in range(GROUP_ENTRIES + 1)]
    used = fresh()
    first_pass = [forward(used, inputs, t, frames=True) for t in ts]
    want = forward(fresh(), inputs, ts[0], frames=True)
    assert torch.isfinite(want).all() and not torch.equal(want, first_pass[1])
    assert torch.equal(first_pass[0], want)
    assert torch.equal(forward(used, inputs, ts[0], frames=True), want)                      # its slot was overwritten by the ninth matrix
    assert torch.equal(first_pass[-1], forward(fresh(), inputs, ts[-1], frames=True))
