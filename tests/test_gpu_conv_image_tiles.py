"""-m gpu: the image-tile map of the plain forward / input-gradient launches (conv_mfma.hip; drs_debug_conv_image_tiles).

An M tile of the map is the same Pc = 128 >> g columns of one image row of 2^g images; tap rows AND tap columns that meet only the
zero halo for the whole tile are left out.  Every output element keeps its K order and the skipped products are exact zeros, so `out`
must be BITWISE what the spatial tiles give with every tap multiplied.  A launch that writes per-tile batch-norm statistics keeps the
spatial tiles (other tiles would group other pixels into the partials): its slab is the bits of today's.  Shapes: the smallest at which each mechanism can go wrong (see SHAPES).  Development library, stream-K off so that the
tiny launches stay plain.
"""
import numpy as np
import pytest
import torch

from oracle import nets as onets
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

from gpu_util import DEV, conv_stats_moments, rel_err, stream   # noqa: E402

# (B, S, k, rate, cin, cout, g)
SHAPES = [
    (128, 8, 3, 8, 32, 64, 7),        # the rate reaches the side: only a few taps are live anywhere
    (128, 2, 4, 3, 64, 128, 7),       # even kernel whose live tap range is EMPTY for some positions: the all-taps guard
    (128, 16, 4, 3, 64, 128, 7),      # asymmetric 4|5 pad: forward with pad_before, input gradient with pad_after
    (128, 16, 5, 2, 64, 64, 7),
    (256, 8, 3, 5, 128, 192, 7),      # two image groups, the 192-wide tile
    (64, 16, 3, 6, 192, 256, 6),      # Pc = 2, two column tiles, six channel chunks
    (64, 16, 3, 6, 192, 256, 5),      # Pc = 4
    (32, 12, 3, 7, 64, 128, 5),       # a tile count that is no multiple of 8
]


@pytest.fixture()
def dev_lib():
    from drs_amd import _lib
    d = _lib.dev()
    old = (d.drs_debug_conv_image_tiles(-1), d.drs_debug_conv_splitk(-1), d.drs_debug_skip_taps(-1))
    try:
        d.drs_debug_conv_splitk(0)
        yield d
    finally:
        d.drs_debug_conv_image_tiles(old[0])
        d.drs_debug_conv_splitk(old[1])
        d.drs_debug_skip_taps(old[2])


def _padded(x, P):
    return torch.nn.functional.pad(x, (0, 0, P, P, P, P)).contiguous()


def _forward(d, xp, B, S, P, w, bias, k, rate, pad, cin, cout, g, skip, acc_into=None, want_stats=False):
    """one launch on the development library; returns (out, statistics slab or None) -- or, accumulate = 1, the [M][ld] slab whose
    channel slice [32, 32 + cout) the launch added its sums to (bias included)"""
    M = B * S * S
    d.drs_debug_conv_image_tiles(g)
    d.drs_debug_skip_taps(skip)
    if acc_into is None:
        mt = d.query("drs_conv_mtile", cout)
        out = torch.full((M, cout), 7.0, device=DEV)
        stats = torch.zeros((M // mt) * cout * 2, device=DEV) if want_stats else None
        d.call("drs_conv_forward", xp.data_ptr(), B, S, P, cin, 0, w.data_ptr(), bias.data_ptr() if bias is not None else None, k, rate, pad,
               cin, cout, out.data_ptr(), cout, 0, 0, stats.data_ptr() if want_stats else None, stream())
        torch.cuda.synchronize()
        return out, stats
    out = acc_into.clone()
    d.call("drs_conv_forward", xp.data_ptr(), B, S, P, cin, 0, w.data_ptr(), bias.data_ptr(), k, rate, pad, cin, cout, out.data_ptr(),
           out.shape[1], 32, 1, None, stream())
    torch.cuda.synchronize()
    return out, None


@pytest.mark.parametrize("B,S,k,rate,cin,cout,g", SHAPES)
def test_image_tiles_give_the_bits_of_spatial_tiles_and_match_the_oracle(dev_lib, B, S, k, rate, cin, cout, g):
    d = dev_lib
    M = B * S * S
    pb, pa = onets.same_pad(k, rate)
    P = max(pb, pa)
    d.drs_debug_conv_image_tiles(g)
    assert d.drs_debug_conv_order_image(B, S, k, rate, pb, cin, cout, None, 0) == (M // 128) * (cout // (192 if cout == 192 else 128 if cout % 128 == 0 else 64))
    gen = torch.Generator(device=DEV).manual_seed(100 * k + rate + S + g)
    x = torch.randn(B, S, S, cin, device=DEV, generator=gen)
    w = torch.randn(k, k, cin, cout, device=DEV, generator=gen) / (k * k * cin) ** 0.5
    bias = torch.randn(cout, device=DEV, generator=gen)
    xp = _padded(x, P)
    # today's map with every tap multiplied / image tiles with the all-halo taps left out, twice
    ref_out, ref_stats = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, 0, 0, want_stats=True)
    out, _ = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, g, 1)
    out2, _ = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, g, 1)
    assert torch.equal(out, ref_out)
    assert torch.equal(out, out2)
    # ... and with every tap multiplied on image tiles
    out3, _ = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, g, 0)
    assert torch.equal(out, out3)
    # a launch that writes tile statistics, with the map forced: out and the slab are the bits of today's, run after run
    outs, stats = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, g, 1, want_stats=True)
    outs2, stats2 = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, g, 1, want_stats=True)
    assert torch.equal(outs, ref_out) and torch.equal(stats, ref_stats)
    assert torch.equal(outs, outs2) and torch.equal(stats, stats2)
    # accumulate = 1 into a non-zero slice of a wider slab
    slab0 = torch.randn(M, cout + 64, device=DEV, generator=gen)
    acc_ref, _ = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, 0, 0, acc_into=slab0)
    acc, _ = _forward(d, xp, B, S, P, w, bias, k, rate, pb, cin, cout, g, 1, acc_into=slab0)
    assert torch.equal(acc, acc_ref)
    assert torch.equal(acc[:, :32], slab0[:, :32]) and torch.equal(acc[:, 32 + cout:], slab0[:, 32 + cout:])
    assert not torch.equal(acc[:, 32:32 + cout], slab0[:, 32:32 + cout])
    # the fp64 oracle convolution
    x64, w64 = x.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    ref = T.conv2d_same(x64, w64, rate) + bias.cpu().numpy().astype(np.float64)
    assert rel_err(out.view(B, S, S, cout).cpu().numpy(), ref) < 1e-5
    # the statistics slab reduces to the moments of out
    mt = d.query("drs_conv_mtile", cout)
    sv = conv_stats_moments(d, stats, M, mt, cout)
    y64 = out.double()
    mean = y64.mean(0).cpu().numpy()
    var = y64.var(0, unbiased=False).cpu().numpy()
    np.testing.assert_allclose(sv[:, 0] / M, mean, rtol=0, atol=1e-6 * np.abs(mean).max() + 1e-7)
    np.testing.assert_allclose(sv[:, 1] / M - (sv[:, 0] / M) ** 2, var, rtol=2e-6)
    if k % 2 == 0 and S == 16:
        # input gradient: the same launch on the output gradient with the flipped, transposed filter and pad_before := pad_after
        assert pa == pb + 1
        gr = torch.randn(B, S, S, cout, device=DEV, generator=gen)
        gp = _padded(gr, P)
        wt = torch.empty(w.numel(), device=DEV)
        d.call("drs_filter_flip_transpose", w.data_ptr(), wt.data_ptr(), k, cin, cout, stream())
        gx_ref, _ = _forward(d, gp, B, S, P, wt, None, k, rate, pa, cout, cin, 0, 0)
        gx, _ = _forward(d, gp, B, S, P, wt, None, k, rate, pa, cout, cin, g, 1)
        assert torch.equal(gx, gx_ref)
        gx64, _ = T.conv2d_same_bwd(x64, w64, rate, gr.cpu().numpy().astype(np.float64))
        assert rel_err(gx.view(B, S, S, cin).cpu().numpy(), gx64) < 1e-5


ENGINE_CASE = ("dilated_grsl_rate8", 5, 6, 32, 16)          # net, channels, classes, B, S; 32 images per tile forced


@pytest.fixture()
def engine_runs(dev_lib, monkeypatch):
    """two training steps of the engine case: step engine and op-level launch sequence on image tiles, step engine on spatial tiles"""
    from drs_amd import _lib
    from drs_amd.net import DilatedNet
    d = dev_lib
    monkeypatch.setattr(_lib, "_lib", d.lib)          # the whole net on the development library
    net, ch, K, B, S = ENGINE_CASE
    rng = np.random.default_rng(4)
    feeds = [(rng.normal(size=(B, S * S * ch)).astype(np.float32), rng.integers(0, K, size=(B, S * S))) for _ in range(2)]

    def run(g, engine):
        d.drs_debug_conv_image_tiles(g)
        n = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, engine=engine)
        losses = []
        for x, y in feeds:
            n.feed(x, y, S)
            out = n.train_step(B, S, 0.01)
            torch.cuda.synchronize()
            losses.append(n.loss_value(out["loss_parts"]))
        return n, losses

    d.drs_debug_conv_image_tiles(5)
    assert d.drs_debug_conv_order_image(B, S, 3, 8, 8, 256, 256, None, 0) > 0          # conv8 of this net does take the map
    runs = {"engine": run(5, True), "oplevel": run(5, False), "spatial": run(0, True)}
    yield runs
    runs.clear()


def test_engine_on_image_tiles_equals_the_op_level_path_and_the_spatial_tiles(engine_runs):
    """the step engine and the op-level launch sequence agree bit for bit with the map forced (the input gradients of conv2..conv8 then
    run on image tiles), as they do on spatial tiles; against the same two steps with the map off the loss and every variable agree to
    the tolerances test_gpu_net.py holds the net to against the oracle -- in fact bit for bit: no convolution output changes and the
    statistics launches keep their tiles"""
    (a, la), (b, lb), (c, lc) = engine_runs["engine"], engine_runs["oplevel"], engine_runs["spatial"]
    for name in ("params", "grads", "mom", "bn"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert la == lb
    for x, y in zip(la, lc):
        assert abs(x - y) < 1e-4 * abs(y)
    for n in a.plan.offsets:
        if n.endswith("/biases") and n != "conv_classifier/biases":
            np.testing.assert_array_equal(a.get_variable(n), c.get_variable(n))          # cancelled by the batch-norm mean: never move
        else:
            assert rel_err(a.get_variable(n), c.get_variable(n)) < 1e-4, n
    for n in a.variable_names():
        if "moving" in n:
            assert rel_err(a.get_variable(n), c.get_variable(n)) < 1e-5, n
    for name in ("params", "grads", "mom", "bn"):
        assert torch.equal(getattr(a, name), getattr(c, name)), name
    assert la == lc
