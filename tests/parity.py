"""Gates and window logic shared by the GPU parity tests (not a conftest: plain helpers, imported by name).

tol / no_farther_than_reference are the project's two per-op gates; the window helpers let a test of a tensor too large
for a whole CPU reference compare output windows against the reference run on the matching, zero-filled input crop."""
import numpy as np
import torch


def tol(ref, k=2e-5):
    """Per-op gate against the fp32 oracle: k of max|ref| (at least k) absolute, 1e-5 relative."""
    return dict(atol=k * max(1.0, float(np.abs(ref).max())), rtol=1e-5)


def ref_errors(a, ref32, ref64):
    """(|a - fp64|, |fp32 reference - fp64|), both as max over the tensor relative to max|fp64|."""
    scale = float(np.abs(ref64).max())
    e_hip = float(np.abs(a.astype(np.float64) - ref64).max()) / scale
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale
    return e_hip, e_ref


def within_reference(e_hip, e_ref, floor=2e-6, margin=4.0):
    """The rule itself on the two figures of ref_errors, for a test that collects failures before it asserts."""
    return e_hip <= margin * e_ref + floor


def no_farther_than_reference(a, ref32, ref64, floor=2e-6, margin=4.0):
    """|HIP - fp64| <= margin * |reference fp32 - fp64| + floor * max|fp64|: the HIP(+MIOpen) result is as close to the
    exact value as the reference's own fp32 result (fixtures: tools/make_golden.py gen_fp64)."""
    e_hip, e_ref = ref_errors(a, ref32, ref64)
    assert within_reference(e_hip, e_ref, floor, margin), (e_hip, e_ref)


def closer_to_fp64(tag, a, ref32, ref64, ref_name='reference32'):
    """Prints both errors of ref_errors as `{tag}: |HIP-fp64| ...  |{ref_name}-fp64| ...` (the PARITY / GLUE lines of the
    logs), then holds `a` to no_farther_than_reference with its defaults."""
    e_hip, e_ref = ref_errors(a, ref32, ref64)
    print(f'{tag}: |HIP-fp64| {e_hip:.3e}  |{ref_name}-fp64| {e_ref:.3e}', flush=True)
    no_farther_than_reference(a, ref32, ref64)


def crop(t, y0, x0, h, w):
    """t[..., y0:y0+h, x0:x0+w] as a CPU tensor, zero where the window leaves the tensor (t may live on the GPU)."""
    th, tw = t.shape[-2:]
    out = torch.zeros(*t.shape[:-2], h, w, dtype=t.dtype)
    sy0, sx0, sy1, sx1 = max(y0, 0), max(x0, 0), min(y0 + h, th), min(x0 + w, tw)
    if sy1 > sy0 and sx1 > sx0:
        out[..., sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = t[..., sy0:sy1, sx0:sx1].cpu()
    return out


def input_window(mode, y0, x0, wh, ww, blur=False):
    """Input crop (iy0, ix0, ih, iw) that determines the output window [y0, y0+wh) x [x0, x0+ww), and the offset (oy, ox)
    of that window in the output computed from the crop alone.
    mode 0: plain 3x3 conv, out[y,x] <- in[y-1..y+1, x-1..x+1].
    mode 1: stride-2 transposed 3x3 conv, out[Y,X] <- in[(Y-2)/2 .. Y/2]; window start even.  blur=True: the output of
    the whole upsampling layer (transposed conv, then the 4-tap FIR with pad (1,1), or the 4-tap pad-(2,1) upsample of a
    ToRGB skip): out[Y] <- conv rows Y-1..Y+2 <- in[(Y-3)/2 .. (Y+2)/2], so the crop takes one more row and column on
    each side."""
    if mode == 0:
        return y0 - 1, x0 - 1, wh + 2, ww + 2, 1, 1
    assert mode == 1 and y0 % 2 == 0 and x0 % 2 == 0
    h = 2 if blur else 1
    iy0, ix0 = y0 // 2 - h, x0 // 2 - h
    return iy0, ix0, (wh + 1) // 2 + 2 * h, (ww + 1) // 2 + 2 * h, y0 - 2 * iy0, x0 - 2 * ix0


def window_check(xd, wgt, s, y, mode, y0, x0, wh, ww):
    """Window of a raw modulated conv (demodulated) against the C oracle run on the input crop."""
    from oracle import c_oracle
    iy0, ix0, ih, iw, oy, ox = input_window(mode, y0, x0, wh, ww)
    ref = c_oracle.modulated_conv2d(crop(xd, iy0, ix0, ih, iw).numpy(), wgt.numpy(), s.numpy(), mode=mode, demodulate=True)
    ref = ref[:, :, oy:oy + wh, ox:ox + ww]       # mode 1: crop row r holds input row iy0 + r, output row Y = 2*(iy0 + r) + ky
    got = y[:, :, y0:y0 + wh, x0:x0 + ww].cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, **tol(ref))


def img_close(a, sub, st, stride, sub64=None, rel=1e-4):
    """End-to-end image gates: the strided sample within rel of max|reference| of the reference's fp32 image (BASELINE.md
    §4), no farther from its float64 image than the reference's own fp32 image (when sub64 is given), and the whole-image
    statistics (mean, mean |.|, sum of squares; tools/make_golden.py stats)."""
    scale = float(np.abs(sub).max())
    np.testing.assert_allclose(a[..., ::stride, ::stride], sub, atol=rel * scale, rtol=rel)
    if sub64 is not None:
        no_farther_than_reference(a[..., ::stride, ::stride], sub, sub64)
    a64 = a.astype(np.float64)
    np.testing.assert_allclose([a64.mean(), np.abs(a64).mean()], st[:2], atol=rel * scale, rtol=rel)
    np.testing.assert_allclose((a64 * a64).sum(), st[4], rtol=10 * rel)
