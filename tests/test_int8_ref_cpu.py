"""CPU suite: tests/int8_ref.py, the reference the GPU tests of the int8 (W8A8) layers compare against (include/ltxhip_int8.h):
the round trip of the row quantisation, the exact product, and the oracle under the w8a8 context."""
import torch

import int8_ref as R
import ltx_oracle as O

CFG = dict(in_channels=16, out_channels=16, num_attention_heads=4, attention_head_dim=32, cross_attention_dim=128, num_layers=3, caption_channels=64)


def test_quant_rows_round_trip_and_edge_rows():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, 144, generator=g).bfloat16()
    x[2] = 0                                                            # a zero row
    x[3, 7] = 1e4                                                       # one outlier 1e4 times the rest
    x[4] = torch.tensor([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5] * 18).bfloat16()      # amax 127: inv = 1, the products are exact half-way cases
    q, s = R.quant_rows(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and q.shape == x.shape and s.shape == (9,)
    xf = x.float()
    sd, amax = s.double()[:, None], xf.double().abs().amax(-1, keepdim=True)
    assert bool(((q.double() * sd - xf.double()).abs() <= sd / 2 + 3 * R.U * amax).all())      # |q s - x| <= s / 2 (+ the f32 roundings of inv, the product and s)
    nz = [i for i in range(9) if i != 2]
    assert bool((q[nz].abs().amax(-1) == 127).all()) and int(q.min()) >= -127
    assert bool((q[2] == 0).all()) and float(s[2]) == 0.0
    assert q[4, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 64]          # half-way cases go to even
    assert torch.equal(s, xf.abs().amax(-1) / torch.tensor(127.0))
    assert int(q[3].abs().sum()) == 127                                 # the outlier row: everything else rounds to zero


def test_exact_product_and_epilogues():
    g = torch.Generator().manual_seed(2)
    qa = torch.randint(-127, 128, (5, 32), generator=g).to(torch.int8); qw = torch.randint(-127, 128, (8, 32), generator=g).to(torch.int8)
    acc = R.acc_i8(qa, qw)
    assert torch.equal(acc, (qa.long() @ qw.long().t()).double())
    sa = torch.rand(5, generator=g) + 0.5; sw = torch.rand(8, generator=g) + 0.5; bias = torch.randn(8, generator=g)
    resid = torch.randn(5, 8, generator=g); gate = torch.randn(2, 8, generator=g)
    v, gv = R.gemm_i8(qa, sa, qw, sw, bias, 0)
    assert torch.allclose(v, acc * sa.double()[:, None] * sw.double()[None, :] + bias.double()) and bool((gv > 0).all())
    assert torch.allclose(R.gemm_i8(qa, sa, qw, sw, bias, 3, resid)[0], v + resid.double())
    rows = torch.tensor([0, 0, 0, 1, 1])
    assert torch.allclose(R.gemm_i8(qa, sa, qw, sw, bias, 2, resid, gate, 3)[0], resid.double() + gate.double()[rows] * v)
    assert torch.allclose(R.gemm_i8(qa, sa, qw, sw, bias, 1)[0].float(), O.gelu_approximate(v.float()), atol=1e-3, rtol=1e-5)


def test_rownorm_quant_follows_the_f64_norm():
    g = torch.Generator().manual_seed(3)
    h = torch.randn(12, 256, generator=g).bfloat16(); shift = torch.randn(3, 256, generator=g); scale = 0.3 * torch.randn(3, 256, generator=g)
    q, s = R.rownorm_quant(h, shift, scale, 4, 1e-6)
    n, gn = R.rownorm64(h, shift, scale, 4, 1e-6)
    amax = n.abs().amax(-1)
    assert bool(((q.double() * s.double()[:, None] - n).abs() <= s.double()[:, None] / 2 + gn + 4 * R.U * amax[:, None]).all())
    assert bool(((s.double() - amax / 127).abs() <= (gn.amax(-1) + 2 * R.U * amax) / 127).all())
    # the exact case: h = +-1, eps = 0, integer tables - n is an integer, q and scale follow exactly
    h1 = (torch.randint(0, 2, (6, 256), generator=g) * 2 - 1).bfloat16()
    sc1 = torch.randint(-3, 4, (2, 256), generator=g).float(); sh1 = torch.randint(-5, 6, (2, 256), generator=g).float()
    q1, s1 = R.rownorm_quant(h1, sh1, sc1, 3, 0.0)
    n1 = h1.float() * (1 + sc1[torch.arange(6) // 3]) + sh1[torch.arange(6) // 3]
    qe, se = R.quant_rows(n1)
    assert torch.equal(q1, qe) and torch.equal(s1, se)


def test_w8a8_context_hits_and_mask_zero_is_the_oracle():
    cfg = O.DitConfig(**CFG)
    w = {k: v.bfloat16().float() for k, v in O.synth_weights(O.dit_weight_shapes(cfg), seed=5).items()}
    B, F, H, W, K = 2, 2, 3, 4, 8
    g = torch.Generator().manual_seed(6)
    hidden = torch.randn(B, F * H * W, 16, generator=g); enc = torch.randn(B, K, 64, generator=g)
    mask = torch.ones(B, K); t = torch.tensor([896.0, 640.0])
    fwd = lambda: O.dit_forward(w, cfg, hidden, enc, t, mask, F, H, W)
    plain = fwd()
    with R.w8a8(w, 0) as st:
        y0 = fwd()
    assert st["hits"] == 0 and torch.equal(y0, plain)                  # mask 0: the oracle bit for bit
    with R.w8a8(w, R.I8_ALL) as st:
        y8 = fwd()
    assert st["hits"] == 18                                             # three blocks x (q, k, v, to_out, ff1, ff2)
    assert O.linear.__module__ == "ltx_oracle" and torch.equal(fwd(), plain)      # the context restores the oracle
    assert not torch.equal(y8, plain) and torch.isfinite(y8).all()
    d = float((y8 - plain).norm() / plain.norm())
    assert d < 0.1, d                                                   # a quantisation's distance, not another function
    with R.w8a8(w, R.I8_ALL, [0, R.I8_FF1 | R.I8_FF2, R.I8_QKV]) as st:
        fwd()
    assert st["hits"] == 2 + 3
    with R.w8a8(w, R.I8_TO_OUT) as st:
        fwd()
    assert st["hits"] == 3
