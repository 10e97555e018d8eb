"""The fused L-BFGS step and the training loop's EMA and loss-row kernels: csrc/lbfgs.hip, train_loop.hip."""
import ctypes

from .core import check, FMGAN_EINVAL, fp, launching, lib, require_f32_gpu, require_gpu


# ----------------------------------------------------------------------------- L-BFGS (csrc/lbfgs.hip)
# The five launches of a fused FullBatchLBFGS step over the buffers of an op.lbfgs.FusedState `s` (it has made the device,
# dtype and layout checks); `table`: the ctypes segment table of lbfgs_segments.
def lbfgs_segments(params):
    """(table, nseg) for the entry points: 3 long long per parameter, {parameter address, gradient address or 0, numel}."""
    vals = []
    for p in params:
        vals += [p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr(), p.numel()]
    return (ctypes.c_longlong * len(vals))(*vals), len(vals) // 3


def lbfgs_pair(s, table, nseg, t, has_pair):
    with launching(s.g, 'lbfgs_pair', (s.n, s.m, bool(has_pair))) as stream:
        st = lib().fmgan_lbfgs_pair_f32(ctypes.addressof(table), nseg, fp(s.g), fp(s.g_prev), fp(s.d), fp(s.S), fp(s.Y),
                                        s.state.data_ptr(), s.partial.data_ptr(), s.n, s.m, float(t), int(has_pair),
                                        stream)
    check(st, 'lbfgs_pair')


def lbfgs_coeffs(s, t, eps, has_pair):
    with launching(s.g, 'lbfgs_coeffs', (s.n, s.m, bool(has_pair))) as stream:
        st = lib().fmgan_lbfgs_coeffs_f64(s.partial.data_ptr(), s.G.data_ptr(), s.state.data_ptr(), s.record.data_ptr(),
                                          s.coef.data_ptr(), s.n, s.m, float(t), float(eps), int(has_pair), stream)
    check(st, 'lbfgs_coeffs')


def lbfgs_direction(s):
    with launching(s.g, 'lbfgs_direction', (s.n, s.m)) as stream:
        st = lib().fmgan_lbfgs_direction_f32(s.coef.data_ptr(), s.state.data_ptr(), fp(s.S), fp(s.Y), fp(s.g),
                                             fp(s.g_prev), fp(s.d), s.partial.data_ptr(), s.record.data_ptr(), s.n, s.m,
                                             stream)
    check(st, 'lbfgs_direction')


def lbfgs_update(s, table, nseg, a):
    with launching(s.g, 'lbfgs_update', (s.n,)) as stream:
        st = lib().fmgan_lbfgs_update_f32(ctypes.addressof(table), nseg, fp(s.d), float(a), s.n, stream)
    check(st, 'lbfgs_update')


def lbfgs_gather(s, table, nseg):
    with launching(s.g, 'lbfgs_gather', (s.n,)) as stream:
        st = lib().fmgan_lbfgs_gather_f32(ctypes.addressof(table), nseg, fp(s.g_new), fp(s.d), s.partial.data_ptr(),
                                          s.record.data_ptr(), s.n, stream)
    check(st, 'lbfgs_gather')


# ----------------------------------------------------------------------------- training loop (csrc/train_loop.hip)
EMA_CHUNK = 4096                          # elements per block of fmgan_ema_f32 (csrc/train_loop.hip EMA_CHUNK)
LOSS_ROW_COLUMNS = 16                     # pointers of fmgan_loss_ptrs, columns of a ledger row


def ema_blocks(numel):
    return int(lib().fmgan_ema_blocks(int(numel)))


def ema(table, n_entries, total_blocks, decay, numel=0):
    """dst <- decay * dst + (1 - decay) * src over every entry of `table` (a uint8 GPU tensor holding n_entries
    fmgan_ema_entry, built by op.ema.EmaPlan, which has made the device, dtype, layout and overlap checks) in one launch
    on the current stream of the table's device.  decay travels as float(decay) and float(1 - decay), the difference
    taken in double."""
    require_gpu(table, 'table')
    decay = float(decay)
    with launching(table, 'ema', (int(n_entries), int(total_blocks), int(numel))) as stream:
        st = lib().fmgan_ema_f32(table.data_ptr(), int(n_entries), int(total_blocks), ctypes.c_float(decay),
                                 ctypes.c_float(1.0 - decay), stream)
    check(st, 'ema')


def loss_row(values, row):
    """One row of the loss log in one launch: values, at most 16 entries, each None or a one-element float32 tensor on
    row's device; row, a contiguous float32 GPU vector of 16 elements (a row of the ledger's ring).  row[i] = values[i]
    (0.0 for None and for the columns past len(values))."""
    n = len(values)
    if n > LOSS_ROW_COLUMNS:
        check(FMGAN_EINVAL, f'loss_row: {n} values for {LOSS_ROW_COLUMNS} columns')
    require_f32_gpu('loss_row', ((row, 'row'),))
    if row.numel() != LOSS_ROW_COLUMNS:
        raise ValueError(f'loss_row: row of {row.numel()} elements, expected {LOSS_ROW_COLUMNS}')
    ptrs = (ctypes.c_void_p * LOSS_ROW_COLUMNS)()
    for k, v in enumerate(values):
        if v is None:
            continue
        if v.numel() != 1 or v.device != row.device:
            raise RuntimeError(f'loss_row: value {k} must hold one element on {row.device}, got {tuple(v.shape)} on '
                               f'{v.device}')
        ptrs[k] = fp(v)
    with launching(row, 'loss_row', (n,)) as stream:
        st = lib().fmgan_loss_row_f32(ctypes.addressof(ptrs), n, fp(row), stream)
    check(st, 'loss_row')
