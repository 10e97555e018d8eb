"""GPU parity tests at model level: Generator / 3-encoder forward / Discriminator on the HIP path vs the golden
vectors captured from the reference, and gradients (first order, R1- and path-length-style second order) vs
autograd through the CPU oracle."""
import numpy as np
import pytest
import torch

import cases
import launches
import synth
from gpumem import dev
from nets import PinNoise, encoders, load
from parity import img_close, no_farther_than_reference as _no_farther_than_reference, tol as _tol

pytestmark = pytest.mark.gpu


def _fp64():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fp64.npz'))


def _img_close(img, g, name, stride, rel=1e-4):
    f64 = _fp64()
    img_close(img.detach().float().cpu().numpy(), g[name + '/sub'], g[name + '/stats'], stride,
              f64[name + '/sub'] if name + '/sub' in f64.files else None, rel)


@pytest.mark.parametrize('c', cases.GENERATOR_CASES, ids=lambda c: c['name'])
def test_generator_golden(c, golden):
    """End-to-end image tolerance 1e-4 of the image's max-abs; measured on MI355X
    (profiles/r02_parity_errors.md): 1.1e-6 .. 2.6e-6 vs the reference's fp32 output, 0.9e-6 .. 2.1e-6 vs its fp64
    output (the reference's own fp32-vs-fp64 distance: 0.8e-6 .. 1.9e-6)."""
    import stylegan2
    g = golden('generator')
    G = load(stylegan2.Generator(c['size'], 512, c['n_mlp'], generator_net_shape=c['shape']), 'generator', 4)
    with torch.no_grad():
        if c['mode'] == 'latent':
            cin0 = c['shape'][0] if c['shape'] else 512
            lat = synth.tensor(c['name'] + '/latent', (c['b'], G.n_latent, 512)).to(dev())
            tsr = synth.tensor(c['name'] + '/tsr', (c['b'], cin0, 4, 4)).to(dev())
            img = G(None, latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True,
                    external_input_tensor=tsr, randomize_noise=False)
        else:
            img = G([synth.tensor(c['name'] + '/z', (c['b'], 512)).to(dev())], randomize_noise=False)
    _img_close(img, g, c['name'], c['stride'])


def test_generator_graph_path_equals_fused_path(golden):
    """With autograd enabled StyledConv runs conv / noise / act as three ops; the image must not change."""
    import stylegan2
    c = cases.GENERATOR_CASES[0]
    G = load(stylegan2.Generator(c['size'], 512, c['n_mlp'], generator_net_shape=c['shape']), 'generator', 4)
    lat = synth.tensor(c['name'] + '/latent', (c['b'], G.n_latent, 512)).to(dev())
    tsr = synth.tensor(c['name'] + '/tsr', (c['b'], 16, 4, 4)).to(dev())
    kw = dict(latent_styles=[lat], input_is_latent=True, use_external_input_tensor=True, external_input_tensor=tsr,
              randomize_noise=False)
    with torch.no_grad():
        a = G(None, **kw)
    b = G(None, **kw)
    _img_close(b, golden('generator'), c['name'], 1)
    torch.testing.assert_close(a, b.detach(), atol=1e-5, rtol=1e-5)
    rgbs, scalars = G(None, return_rgb_list=True, return_style_scalars=True, **kw)
    assert len(rgbs) == 5 and len(scalars) == G.num_layers + 1
    torch.testing.assert_close(rgbs[-1].detach(), a, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize('c', cases.E2E_CASES, ids=lambda c: c['name'])
def test_forward_inference_3_encoder_golden(c, golden):
    """(photo, render) -> image through encoders (MIOpen) + Generator (HIP kernels) vs the reference."""
    import stylegan2
    from Util.network_util import Forward_Inference_3_Encoder
    g = golden('e2e')
    n_latent = int(np.log2(c['size'])) * 2 - 2
    e_tsr, e_w, e_wp = encoders(n_latent)
    G = load(stylegan2.Generator(c['size'], 512, 8), 'generator', 4)
    p = synth.tensor(c['name'] + '/photo', (c['b'], 3, 256, 256), dist='uniform').to(dev())
    r = synth.tensor(c['name'] + '/render', (c['b'], 3, 256, 256), dist='uniform').to(dev())
    # Tolerances = measured error x ~5 (profiles/r02_parity_errors.md).  Encoders (MIOpen convolutions, summation order
    # differs from the CPU reference): measured 1.5e-7 .. 7.1e-7 of max|out| -> 5e-6.  End-to-end image: BASELINE.md §4
    # asks atol = rtol = 1e-4; measured 1.2e-6 .. 1.8e-6, and 1.1e-5 for the tanh case whose max is 1 -> 5e-5.
    f64 = _fp64()
    with torch.no_grad():
        for net, x, key in ((e_tsr, p, 'e_tsr'), (e_w, r, 'e_w'), (e_wp, p, 'e_wplus')):
            out, ref = net(x).cpu().numpy(), g[f"{c['name']}/{key}"]
            np.testing.assert_allclose(out, ref, atol=5e-6 * np.abs(ref).max(), rtol=1e-4)
            _no_farther_than_reference(out, ref, f64[f"{c['name']}/{key}"])
        img = Forward_Inference_3_Encoder(p, r, e_tsr, e_w, e_wp, PinNoise(G), tsr_encode=c['tsr_encode'],
                                          sliced_layer=c['sliced_layer'], use_tanh=c['use_tanh'])
    _img_close(img, g, c['name'], c['stride'], rel=5e-5)


@pytest.mark.parametrize('c', cases.DISCRIMINATOR_CASES, ids=lambda c: c['name'])
def test_discriminator_golden(c, golden):
    import stylegan2
    g = golden('discriminator')
    D = load(stylegan2.Discriminator(c['size']), 'discriminator', 8)
    x = synth.tensor(c['name'] + '/x', (c['b'], 3, c['size'], c['size']), dist='uniform').to(dev())
    with torch.no_grad():
        y = D(x)
    ref = g[c['name'] + '/out']
    # measured 2.0e-7 .. 5.4e-7 of max|out| (profiles/r02_parity_errors.md) -> 5e-6
    np.testing.assert_allclose(y.cpu().numpy(), ref, atol=5e-6 * np.abs(ref).max(), rtol=1e-4)
    _no_farther_than_reference(y.cpu().numpy(), ref, _fp64()[c['name'] + '/out'])


def test_generator_gradients_and_path_length_vs_oracle():
    """Narrow Generator(32): d(image)/d(latent, tensor, weights) and the in-forward path-length regulariser
    (second order, stylegan2.py:683-688) vs float64 autograd through the CPU oracle."""
    import math
    import stylegan2
    from oracle import torch_oracle as T
    shape = [8, 8, 8, 8, 8, 8, 6, 6]
    G = load(stylegan2.Generator(32, 512, 1, generator_net_shape=shape), 'generator', 12)
    sd64 = {k: v.detach().cpu().double() for k, v in G.state_dict().items()}
    lat = synth.tensor('gg/lat', (2, G.n_latent, 512))
    tsr = synth.tensor('gg/tsr', (2, 8, 4, 4))
    go = synth.tensor('gg/go', (2, 3, 32, 32))
    # oracle
    lo, to = lat.double().requires_grad_(True), tsr.double().requires_grad_(True)
    wkey = 'convs.1.conv.weight'
    sd64[wkey].requires_grad_(True)
    img_o = T.generator_forward(sd64, 32, lo, external_input_tensor=to, noise='buffers')
    glo, gto, gwo = torch.autograd.grad(img_o, (lo, to, sd64[wkey]), go.double(), create_graph=True)
    probe = synth.tensor('gg/probe', (2, 3, 32, 32)).double() / math.sqrt(32 * 32)
    gpl_o, = torch.autograd.grad((img_o * probe).sum(), lo, create_graph=True)
    pl_o = torch.sqrt(gpl_o.pow(2).sum(2).mean(1))
    gpl2_o, = torch.autograd.grad(pl_o.sum(), lo)
    # HIP
    ld, td = lat.to(dev()).requires_grad_(True), tsr.to(dev()).requires_grad_(True)
    img_d = G(None, latent_styles=[ld], input_is_latent=True, use_external_input_tensor=True, external_input_tensor=td,
              randomize_noise=False)
    wd = dict(G.named_parameters())[wkey]
    gld, gtd, gwd = torch.autograd.grad(img_d, (ld, td, wd), go.to(dev()), create_graph=True)

    def close(a, b, k):
        b = b.detach().numpy()
        np.testing.assert_allclose(a.detach().cpu().numpy(), b, atol=k * max(1e-6, float(np.abs(b).max())), rtol=k)

    close(img_d, img_o, 1e-4)
    close(gld, glo, 1e-3)
    close(gtd, gto, 1e-3)
    close(gwd, gwo, 1e-3)
    from Util.training_util import g_path_regularize
    pen_d, mean_d, pl_d = g_path_regularize(img_d, ld, 0.5, probe=synth.tensor('gg/probe', (2, 3, 32, 32)).to(dev()))
    gpl2_d, = torch.autograd.grad(pl_d.sum(), ld, retain_graph=True)
    mean_o = 0.5 + 0.01 * (pl_o.mean() - 0.5)
    np.testing.assert_allclose(mean_d.item(), mean_o.item(), rtol=1e-3)
    np.testing.assert_allclose(pen_d.item(), (pl_o - mean_o).pow(2).mean().item(), rtol=5e-3)
    close(pl_d, pl_o, 1e-3)
    close(gpl2_d, gpl2_o, 5e-3)
    # and the PPL_regularize=True return signature
    out = G(None, latent_styles=[ld], input_is_latent=True, use_external_input_tensor=True, external_input_tensor=td,
            randomize_noise=False, PPL_regularize=True)
    assert isinstance(out, tuple) and tuple(out[1].shape) == (2,)


def test_discriminator_r1_penalty_vs_oracle():
    """R1 (Util/training_util.py:46-52): grad of D(real) w.r.t. the image with create_graph, then backward —
    double-backward through upfirdn2d and fused_leaky_relu on the HIP path."""
    import stylegan2
    from oracle import torch_oracle as T
    D = load(stylegan2.Discriminator(16), 'discriminator', 13)
    sd64 = {k: v.detach().cpu().double() for k, v in D.state_dict().items()}
    x = synth.tensor('r1/x', (4, 3, 16, 16), dist='uniform')
    wkey = 'convs.1.conv2.1.weight'
    sd64[wkey].requires_grad_(True)
    xo = x.double().requires_grad_(True)
    yo = T.discriminator_forward(sd64, xo, 16)
    gxo, = torch.autograd.grad(yo.sum(), xo, create_graph=True)
    r1_o = gxo.pow(2).reshape(4, -1).sum(1).mean()
    gw_o, = torch.autograd.grad(r1_o, sd64[wkey])
    from Util.training_util import d_r1_loss, d_logistic_loss, g_nonsaturating_loss
    xd = x.to(dev()).requires_grad_(True)
    yd = D(xd)
    r1_d = d_r1_loss(yd, xd)
    gw_d, = torch.autograd.grad(r1_d, dict(D.named_parameters())[wkey])
    sp = torch.nn.functional.softplus
    np.testing.assert_allclose(d_logistic_loss(yd[:2], yd[2:]).item(),
                               (sp(-yo[:2]).mean() + sp(yo[2:]).mean()).item(), rtol=1e-4)
    np.testing.assert_allclose(g_nonsaturating_loss(yd).item(), sp(-yo).mean().item(), rtol=1e-4)
    np.testing.assert_allclose(yd.detach().cpu().numpy(), yo.detach().numpy(), atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(r1_d.item(), r1_o.item(), rtol=1e-3)
    ref = gw_o.numpy()
    np.testing.assert_allclose(gw_d.cpu().numpy(), ref, atol=2e-3 * np.abs(ref).max(), rtol=2e-3)


def test_overlapped_and_graphed_forward_equal_serial():
    """Inference issues the ResNet encoders and the RGB branch on side streams, and the whole forward can be replayed
    from a HIP graph.  The Generator (this repo's kernels: no atomics, fixed summation order) must be bit-identical
    run to run, overlapped or not, graphed or not; the full path is compared to tolerance because MIOpen's encoder
    convolutions are themselves not bit-reproducible run to run — also with side streams off: profiles/r02_determinism.md
    keeps the output of tools/exp_determinism.py (e_tsr 1.9e-6, e_wp 3.9e-7, Generator 0.0, streams on and off).  The
    scheduling itself is pinned bit-exactly by test_full_path_is_bit_reproducible_once_encoder_outputs_are_fixed."""
    import stylegan2
    from Util import streams
    from Util.network_util import Forward_Inference_3_Encoder
    from Util.hip_graph import GraphedForward
    e_tsr, e_w, e_wp = encoders(10)
    G = load(stylegan2.Generator(64, 512, 2), 'generator', 4)
    p = synth.tensor('ovl/photo', (2, 3, 256, 256), dist='uniform').to(dev())
    r = synth.tensor('ovl/render', (2, 3, 256, 256), dist='uniform').to(dev())
    lat = synth.tensor('ovl/lat', (2, G.n_latent, 512)).to(dev())
    tsr = synth.tensor('ovl/tsr', (2, 512, 4, 4)).to(dev())
    wrap = PinNoise(G)

    def gen(l, t):
        with torch.no_grad():
            return G(None, latent_styles=[l], input_is_latent=True, use_external_input_tensor=True,
                     external_input_tensor=t, randomize_noise=False)

    def fwd(a, b):
        with torch.no_grad():
            return Forward_Inference_3_Encoder(a, b, e_tsr, e_w, e_wp, wrap)

    try:
        streams.ENABLED = False
        g_serial = gen(lat, tsr).clone()
        f_serial = fwd(p, r).clone()
    finally:
        streams.ENABLED = True
    g_overlap = gen(lat, tsr).clone()
    assert torch.equal(g_overlap, g_serial)
    for _ in range(3):
        assert torch.equal(gen(lat, tsr), g_serial)           # no race: repeated overlapped runs are bit-identical
    gg = GraphedForward(gen, (lat, tsr))
    for _ in range(3):
        assert torch.equal(gg(lat, tsr), g_serial)
    lat2 = synth.tensor('ovl/lat2', (2, G.n_latent, 512)).to(dev())
    assert torch.equal(gg(lat2, tsr), gen(lat2, tsr))          # new inputs are copied into the static buffers
    tol = dict(atol=1e-4 * float(f_serial.abs().max()), rtol=1e-4)
    torch.testing.assert_close(fwd(p, r), f_serial, **tol)
    gf = GraphedForward(fwd, (p, r))
    torch.testing.assert_close(gf(p, r), f_serial, **tol)


def test_pipelined_forward_matches_serial_for_partial_slices_and_tanh():
    """The inference schedule (synthesis network behind per-head events of the pSp encoder, Util/network_util._pipelined)
    must equal the single-stream composition for any sliced_layer subset (W * W+ only on those layers), with tanh,
    and when the generator has fewer layers than the encoder has style heads."""
    import stylegan2
    from Util import streams
    from Util.network_util import Forward_Inference_3_Encoder
    e_tsr, e_w, e_wp = encoders(10)                               # 10 style heads
    G = load(stylegan2.Generator(32, 512, 2), 'generator', 21)    # n_latent = 8 < 10
    wrap = PinNoise(G)
    p = synth.tensor('pipe/photo', (3, 3, 256, 256), dist='uniform').to(dev())
    r = synth.tensor('pipe/render', (3, 3, 256, 256), dist='uniform').to(dev())
    for sliced, tanh in ((None, False), ([0, 3, 4], True), ([], False), (range(2, 20), True)):
        with torch.no_grad():
            fast = Forward_Inference_3_Encoder(p, r, e_tsr, e_w, e_wp, wrap, sliced_layer=sliced, use_tanh=tanh).clone()
            try:
                streams.ENABLED = False
                slow = Forward_Inference_3_Encoder(p, r, e_tsr, e_w, e_wp, wrap, sliced_layer=sliced, use_tanh=tanh)
            finally:
                streams.ENABLED = True
        torch.testing.assert_close(fast, slow, atol=1e-4 * float(slow.abs().max()), rtol=1e-4)
    # render image as the tensor-encoder input
    with torch.no_grad():
        a = Forward_Inference_3_Encoder(p, r, e_tsr, e_w, e_wp, wrap, tsr_encode='Render Image')
        b = Forward_Inference_3_Encoder(r, r, e_tsr, e_w, e_wp, wrap)            # photo := render for E_Tsr only...
    assert tuple(a.shape) == (3, 3, 32, 32) and not torch.equal(a, b)


def test_forward_through_data_parallel_wrappers_equals_bare_modules():
    """The reference calls Forward_Inference_3_Encoder on DataParallel-wrapped networks (train_3_encoder.py:355-362 —
    it even requires `.module` on the generator).  Miscellaneous.distributed.data_parallel returns such
    wrappers; the inference schedule must see through them and give the bare modules' result."""
    import stylegan2
    from Miscellaneous import distributed as D
    from Util.network_util import Forward_Inference_3_Encoder
    e_tsr, e_w, e_wp = encoders(8)
    G = load(stylegan2.Generator(32, 512, 2), 'generator', 21)
    p = synth.tensor('dpw/photo', (2, 3, 256, 256), dist='uniform').to(dev())
    r = synth.tensor('dpw/render', (2, 3, 256, 256), dist='uniform').to(dev())
    bare = PinNoise(G)
    wrapped = [D.data_parallel(m, dev()) for m in (e_tsr, e_w, e_wp)]
    assert all(hasattr(w, 'module') for w in wrapped)
    with torch.no_grad():
        a = Forward_Inference_3_Encoder(p, r, e_tsr, e_w, e_wp, bare).clone()
        b = Forward_Inference_3_Encoder(p, r, *wrapped, bare)
    torch.testing.assert_close(b, a, atol=1e-5 * float(a.abs().max()), rtol=1e-5)


def test_full_path_is_bit_reproducible_once_encoder_outputs_are_fixed():
    """MIOpen's encoder convolutions are not bit-reproducible run to run even on ONE stream (profiles/r02_determinism.md:
    e_tsr 1.9e-6, e_wp 3.9e-7 between identical calls with side streams off), which is why the full (photo, render)
    path is compared to tolerance.  Everything this repo schedules — the side-stream fork/join of the encoders, the
    per-head events of the pipelined W+ hand-over, co-modulation, the synthesis network with its RGB side stream — must
    itself be exact: with the encoders replaced by modules that return fixed tensors the overlapped, pipelined forward
    is bit-identical to the single-stream one, every time."""
    import stylegan2
    from Util import streams
    from Util.network_util import Forward_Inference_3_Encoder
    from Util.streams import run_deferred, side_streams
    G = load(stylegan2.Generator(64, 512, 2), 'generator', 4)
    n = G.n_latent
    tsr = synth.tensor('fix/tsr', (2, 512, 4, 4)).to(dev())
    wv = synth.tensor('fix/w', (2, 512)).to(dev())
    wp = synth.tensor('fix/wp', (2, n, 512)).to(dev())
    x = synth.tensor('fix/x', (2, 3, 256, 256), dist='uniform').to(dev())

    class Fixed(torch.nn.Module):
        def __init__(self, out):
            super().__init__()
            self.out = out

        def forward(self, _):
            return self.out + 0.0              # a real launch on whatever stream the caller put us on

    class FixedHeads(Fixed):
        def forward_deferred(self, _):
            ss = side_streams(self.out.device, 2, 'psp-heads')
            if not streams.overlap_ok(self.out):
                return [((lambda: None), self.out[:, i] + 0.0) for i in range(n)]
            return [run_deferred(ss[i % 2], lambda t: t + 0.0, self.out[:, i]) for i in range(n)]

    nets = (Fixed(tsr), Fixed(wv), FixedHeads(wp))

    def fwd(sliced):
        with torch.no_grad():
            return Forward_Inference_3_Encoder(x, x, *nets, PinNoise(G), sliced_layer=sliced).clone()

    for sliced in (None, [1, 4, 5]):
        try:
            streams.ENABLED = False
            serial = fwd(sliced)
        finally:
            streams.ENABLED = True
        for _ in range(4):
            assert torch.equal(fwd(sliced), serial)


def test_placement_workspaces_do_not_change_results_or_leak(monkeypatch):
    """op/placement.py: the persistent, placement-selected (intermediate, output) pairs of the large upsampling layers.
    Same bits as with fresh allocations; the image returned is always a fresh tensor and survives the next forward; a
    layer called on its own never hands out a persistent tensor; selection happened for exactly the layers above 256 MiB."""
    import stylegan2
    from op import placement
    G = load(stylegan2.Generator(256, 512, 2), 'generator', 4)
    b = 32
    lat = synth.tensor('pl/lat', (b, G.n_latent, 512)).to(dev())
    lat2 = synth.tensor('pl/lat2', (b, G.n_latent, 512)).to(dev())
    tsr = synth.tensor('pl/tsr', (b, 512, 4, 4)).to(dev())
    kw = dict(input_is_latent=True, use_external_input_tensor=True, external_input_tensor=tsr, randomize_noise=False)
    placement.forget()
    with torch.no_grad():
        monkeypatch.setattr(placement, 'ENABLED', False)
        ref = G(None, latent_styles=[lat], **kw)
        ref2 = G(None, latent_styles=[lat2], **kw)
        monkeypatch.setattr(placement, 'ENABLED', True)
        img = G(None, latent_styles=[lat], **kw)
        keep = img.clone()
        img2 = G(None, latent_styles=[lat2], **kw)
    assert torch.equal(img, ref) and torch.equal(img2, ref2)
    assert img.data_ptr() != img2.data_ptr() and torch.equal(img, keep)       # the first image was not overwritten
    owners = [m for m in G.modules() if m in placement._STORE]
    sizes = sorted(ws.buf.numel() * 4 for m in owners for ws in placement._STORE[m].values())
    assert len(sizes) == 3 and sizes[0] >= placement.MIN_BYTES, sizes         # the 64^2, 128^2 and 256^2 upsampling layers
    assert all(2 <= ws.tried <= 2 * placement.MAX_CANDIDATES for m in owners for ws in placement._STORE[m].values())
    # a StyledConv called directly (no network scope) returns fresh tensors
    sc = G.convs[-2]
    x = synth.tensor('pl/x', (b, sc.conv.in_channel, 128, 128)).to(dev())
    with torch.no_grad():
        y1 = sc(x, lat[:, 0])
        y2 = sc(x * 0.5, lat[:, 0])
    assert y1.data_ptr() != y2.data_ptr() and not torch.equal(y1, y2)
    placement.forget()


def _styled_up(blur_kernel, name):
    """A small upsampling StyledConv with synthetic weights, its inputs, and the fp32 oracle's output for them."""
    import stylegan2
    from oracle import torch_oracle as T
    b, cin, cout, h = 2, 16, 24, 40
    sc = stylegan2.StyledConv(cin, cout, 3, 512, upsample=True, blur_kernel=list(blur_kernel))
    sd = synth.state_dict('generator', sc.state_dict(), seed=6)
    sc.load_state_dict(sd)
    x = synth.tensor(name + '/x', (b, cin, h, h))
    lat = synth.tensor(name + '/lat', (b, 512))
    noise = synth.tensor(name + '/noise', (b, 1, 2 * h, 2 * h))
    with torch.no_grad():
        ref = T.styled_conv({'L.' + k: v for k, v in sd.items()}, 'L', x, lat, noise, True, blur_kernel=tuple(blur_kernel))
    return sc.to(dev()).eval(), x.to(dev()), lat.to(dev()), noise.to(dev()), ref.numpy()


def test_blur_the_fused_kernel_does_not_serve_inside_a_placement_scope(monkeypatch):
    """StyledConv(upsample=True, blur_kernel=[1,4,6,4,1]): the fused blur + noise + bias + act kernels take FIRs of at most
    4 taps (tests/test_abi_host.py), so this layer runs the two-pass form.  Inside placement.scope(), with an intermediate
    above placement.MIN_BYTES, the layer used to hand its producer/consumer pair to placement.workspace(): the selection
    timed a consumer that launched nothing and the layer returned the never-written persistent output.  MIN_BYTES is
    patched down to 1 MiB here (the real threshold needs B = 8 at 512^2) — the branch taken is the same.  Gates: the fp32
    oracle with the same blur_kernel at the per-op tolerance, and the same bits as the call outside any scope."""
    from op import placement
    sc, x, lat, noise, ref = _styled_up([1, 4, 6, 4, 1], 'pl5')
    h = x.shape[2]
    assert 4 * x.shape[0] * sc.conv.out_channel * (2 * h + 1) * (2 * h + 1) >= 1 << 20
    monkeypatch.setattr(placement, 'MIN_BYTES', 1 << 20)
    monkeypatch.setattr(placement, 'ENABLED', True)
    placement.forget()
    with torch.no_grad():
        off = sc(x, lat, noise=noise)
        with launches.observed() as obs, placement.scope():
            on = sc(x, lat, noise=noise).clone()
    np.testing.assert_allclose(on.cpu().numpy(), ref, **_tol(ref))
    assert torch.equal(on, off)
    # no workspace was selected for a pair whose consumer has no kernel; the fused blur was asked once and declined, then
    # the FIR and the epilogue ran as two passes
    assert sc not in placement._STORE
    assert obs.names == ['modconv2d', 'upfirdn2d', 'upfirdn2d', 'noise_bias_act'], obs.names
    placement.forget()


def test_default_blur_inside_a_placement_scope_keeps_its_two_launches(monkeypatch):
    """The same layer with the default [1,3,3,1] blur (served by the fused kernel), MIN_BYTES patched down as above: a
    workspace is selected on the first call; every later call is exactly producer + fused blur into the persistent pair,
    with the oracle's values and the bits of the call outside the scope."""
    from op import placement
    sc, x, lat, noise, ref = _styled_up([1, 3, 3, 1], 'pl4')
    monkeypatch.setattr(placement, 'MIN_BYTES', 1 << 20)
    monkeypatch.setattr(placement, 'ENABLED', True)
    placement.forget()
    with torch.no_grad():
        off = sc(x, lat, noise=noise)
        with placement.scope():
            first = sc(x, lat, noise=noise).clone()
            with launches.observed() as obs:
                again = sc(x, lat, noise=noise)
    ws, = placement._STORE[sc].values()
    assert again.data_ptr() == ws.out.data_ptr()
    assert obs.names == ['modconv2d', 'upfirdn2d'], obs.names
    np.testing.assert_allclose(again.cpu().numpy(), ref, **_tol(ref))
    assert torch.equal(first, off) and torch.equal(again, off)
    placement.forget()
