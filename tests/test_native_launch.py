"""op/_native/core.py's launch bracket (`launching`) and status function (`served`): what an observer sees of a wrapper — one
begin / end pair per bracket, with the wrapper's (name, info), also round a multi-launch wrapper and round a launch the
library declines — and how a status becomes True / False / RuntimeError."""
import numpy as np
import pytest
import torch

import launches
import synth
from parity import tol as _tol


def test_served_interprets_the_status():
    from op import _native
    L = _native.lib()
    assert (_native.FMGAN_OK, _native.FMGAN_EUNSUPPORTED) == (0, -2)            # include/fmgan_hip.h
    assert _native.served(_native.FMGAN_OK, 'x') is True
    assert _native.served(_native.FMGAN_EUNSUPPORTED, 'x') is False
    einval = -1
    text = L.fmgan_status_string(einval).decode()
    assert text and text != L.fmgan_status_string(0).decode()
    for fn in (_native.served, _native.check):
        with pytest.raises(RuntimeError) as e, launches.observed() as rec:
            assert _native.core._observer is rec
            fn(einval, 'some_launch')
        assert str(e.value) == f'some_launch: {text} (status {einval})'
        assert isinstance(_native.core._observer, _native.core._NullObserver)         # back after a body that raised


class _Recorder:
    """Local, not launches.Recorder: this one tests the bracket itself (end() gets the token its begin() returned)."""

    def __init__(self):
        self.events = []

    def begin(self, name, info):
        self.events.append(('begin', name, info))
        return len(self.events)

    def end(self, token):
        assert token == len(self.events)          # the token of this bracket's begin, and nothing recorded in between
        self.events.append(('end',))


def _recorded(fn):
    """(fn(), the events an observer saw during it); the null observer is back afterwards, whatever fn did."""
    with launches.observed(_Recorder()) as rec:
        return fn(), rec.events


@pytest.mark.gpu
def test_single_launch_gives_one_bracket():
    from op import _native
    d = torch.device('cuda', 0)
    x = synth.tensor('launch/nba/x', (1, 4, 8, 8)).to(d)
    bias = synth.tensor('launch/nba/b', (4,)).to(d)
    y, events = _recorded(lambda: _native.noise_bias_act(x, None, None, bias, 0.2, 2 ** 0.5))
    assert events == [('begin', 'noise_bias_act', (256, 4)), ('end',)]
    pre = x + bias[None, :, None, None]
    # three fp32 roundings (add, slope, gain) of 2^-24 each, whatever the kernel's association: 1e-6 covers them
    torch.testing.assert_close(y, torch.where(pre > 0, pre, pre * 0.2) * 2 ** 0.5, rtol=1e-6, atol=1e-6)
    assert isinstance(_native.core._observer, _native.core._NullObserver)


@pytest.mark.gpu
def test_winograd_form_is_one_bracket_round_three_launches():
    from op import _native
    from oracle import c_oracle
    d = torch.device('cuda', 0)
    b, c, h = 1, 8, 16
    x = synth.tensor('launch/wino/x', (b, c, h, h))
    wgt = synth.tensor('launch/wino/w', (c, c, 3, 3))
    s = synth.tensor('launch/wino/s', (b, c), shift=1.0, scale=0.5)
    scale = 1.0 / np.sqrt(c * 9)
    ref = c_oracle.modulated_conv2d(x.numpy(), wgt.numpy(), s.numpy(), mode=0, demodulate=True)
    xd, wd, sd = x.to(d), wgt.to(d), s.to(d)
    wt = _native.modconv_weight_prep(wd, scale)
    dm = _native.modconv_demod(wd, sd, scale)
    u = _native.wino_weight(wt)
    y, events = _recorded(lambda: _native.modconv2d_winograd(xd, wt, sd, dm, u=u))
    assert events == [('begin', 'modconv2d_winograd', (b, c, c, h, h, 0)), ('end',)]
    yd, events = _recorded(lambda: _native.modconv2d(xd, wt, sd, dm, 0))
    assert events == [('begin', 'modconv2d', (b, c, c, h, h, 0)), ('end',)]
    # tests/test_hip_modconv.py::test_winograd_form_vs_c_oracle: the direct kernel's gate against the oracle, for the pair too
    np.testing.assert_allclose(y.cpu().numpy(), ref, **_tol(ref))
    np.testing.assert_allclose(y.cpu().numpy(), yd.cpu().numpy(), **_tol(ref))


@pytest.mark.gpu
def test_declined_launch_returns_none_with_the_bracket_closed():
    from op import _native
    d = torch.device('cuda', 0)
    x = synth.tensor('launch/bn/x', (1, 6, 4, 4)).to(d).contiguous(memory_format=torch.channels_last)
    bn = tuple(synth.tensor(f'launch/bn/{k}', (6,)).to(d) for k in 'mvgb')
    bn = (bn[0], bn[1].abs() + 0.5, bn[2], bn[3], 1e-5)
    slope = synth.tensor('launch/bn/slope', (6,)).to(d)
    out, events = _recorded(lambda: _native.bn_prelu(x, bn, slope))
    assert out is None                                                          # C % 4 != 0: the library declines
    assert events == [('begin', 'bn_prelu', (1, 6, 4, 4)), ('end',)]
    assert isinstance(_native.core._observer, _native.core._NullObserver)
