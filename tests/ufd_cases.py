"""Case tables of tests/test_hip_upfirdn2d_kernels.py: every fast kernel of csrc/upfirdn2d.hip at the smallest arguments that
reach one of its edges.  Plain data — the CPU suite (tests/test_abi_host.py) replays every row through
fmgan_upfirdn2d_select, so a change of the plan's rules fails there before a GPU sees it.

A row is (kernel, major, in_h, in_w, kh, kw, up, px0, px1, py0, py1): f32, minor 1, down 1, `up` on both axes.  `kernel` is
the header's numbering (0 generic, 1 register row-march, 5 LDS-DMA ring, 2 plane-tile, 3 up=2 polyphase).  The ring is
chosen by address, which a select without pointers cannot see: for a row named 5 the select answers 1 and the test insists
on path 5.  OUT_SIZE holds the (out_h, out_w) each row was written for, worked out by hand from
out = in * up + pad0 + pad1 - taps + 1.  Except for the single-tap rows, pad_x0 != pad_y0 (and pad_x1 != pad_y1 nearly
everywhere): a kernel that read one where it needs the other fails the row.
"""

# ------------------------------------------------------------------------------------------------ kernel 1: row-march
# VEC is 1 below 96 output columns, 2 below 192, else 4; a wave covers 64 * VEC columns (a "strip") and 4 rows at these
# plane counts (the row tile grows only when the grid is large enough, see ROWMARCH_TALL).
ROWMARCH = [
    (1, 2, 9, 70, 4, 4, 1, 0, 3, 2, -1),      # VEC=1, two strips, ragged row tile (7 rows = 4 + 3)
    (1, 3, 6, 120, 3, 2, 1, -2, 1, 3, 0),     # VEC=2, crop on the left
    (1, 1, 4, 200, 1, 4, 1, 3, -1, 0, 0),     # VEC=4, the out_h minimum, odd row length
    (1, 2, 11, 60, 2, 1, 1, 5, 40, -2, 1),    # most lanes' windows wholly right of the image
    (1, 1, 5, 300, 4, 3, 1, 1, 0, 0, 2),      # VEC=4, two strips
    (1, 2, 8, 64, 1, 1, 1, 0, 0, 0, 0),       # narrowest plane, single tap
]
# 4096 planes x 1 strip x 2 row tiles of 32 = 8192 waves = 32 x 256 CUs: the plan keeps 32-row tiles (64-row tiles would
# give 4096 waves) and the march loop takes its back-edge.  On a device with another CU count the test scales `major`
# (rowmarch_tall_major) so that the same inequality holds.
ROWMARCH_TALL = (1, 4096, 65, 65, 4, 4, 1, 2, 0, 0, 2)


def rowmarch_tall_major(cus):
    """Planes at which [., 65, 65] -> [., 64, 64] gets 32-row tiles: major * 1 * 2 >= 32 * cus > major * 1 * 1."""
    return 16 * cus


# ------------------------------------------------------------------------------------------------ kernel 5: LDS-DMA ring
# Inputs in the aligned-row layout (op/_native/conv.py::aligned_rows_buffer(pad0=px0)); out_w % 4 == 0, >= 256, out_h >= 8.
RING = [
    (5, 2, 12, 259, 4, 4, 1, 0, 0, 3, -1),    # 11 rows: an 8-row tile plus a 3-row remainder (the vmcnt(0) steps)
    (5, 2, 9, 254, 3, 4, 1, 3, 2, 0, 3),      # pad_x0 = 3: three masked positions on the left; 10 rows
    (5, 2, 14, 260, 4, 2, 1, 2, -1, -1, 2),   # a second strip of one live lane; rows cropped at the top
]
# pad_x0 < 0 is outside the ring's rules: insisting on path 5 is refused, the automatic launch is the register row-march
RING_REFUSED = (1, 2, 12, 259, 4, 4, 1, -1, 0, 3, -1)

# ------------------------------------------------------------------------------------------------ kernel 2: plane-tile
PLANETILE = [
    (2, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0),        # smallest plane
    (2, 5, 12, 12, 4, 4, 1, -1, 2, 2, -1),    # crop on both axes
    (2, 3, 2, 300, 2, 3, 1, 1, 1, 0, 0),      # wide but out_h < 4, so not row-march
    (2, 2, 256, 48, 3, 4, 1, 0, 2, 1, 1),     # in_h * in_w == 12288 (the bound), pb = 1, 48 KB of LDS
    (2, 40001, 3, 5, 2, 2, 1, 1, 0, 0, 1),    # pb = 64, 626 blocks, the last block holds one plane
    (2, 2, 4, 4, 4, 4, 1, 30, 30, 3, 3),      # almost all zeros
]
PLANETILE_OVER = (0, 2, 241, 51, 4, 4, 1, 1, 0, 0, 1)       # 12291 input elements: one row past the bound, generic kernel
PLANETILE_STRIDED = (2, 5, 9, 9, 4, 4, 1, 2, 1, 0, 3)       # read from an aligned-row buffer (the kernel's strided copy)

# ------------------------------------------------------------------------------------------------ kernel 3: up=2 polyphase
# ufd_up2_f32<PY, PX> is instantiated per parity of (pad_y0, pad_x0); a thread owns 2 rows x 4 columns of the output.
UP2 = [
    (3, 2, 7, 9, 4, 4, 2, 1, 2, 2, 1),        # <0,1>, out_w % 4 == 2
    (3, 3, 5, 3, 3, 4, 2, 2, 0, 1, 1),        # <1,0>, in_w < 4 (scalar row loads only), out_w % 4 == 1
    (3, 1, 8, 33, 4, 2, 2, -1, 2, 0, 3),      # <0,1> from a negative odd pad
    (3, 2, 6, 10, 2, 3, 2, 0, 1, -1, 1),      # <1,0>, odd out_h, out_w % 4 == 3
    (3, 1, 4, 6, 1, 1, 2, 3, 3, 3, 3),        # <1,1>, single tap
]
# 17 x 256 x 512 thread items > 32 x 256 CUs x 256 threads: the grid-stride loop takes a second trip (the production ToRGB
# skip upsample [24,512,512] -> [24,1024,1024] does); the test derives the plane count from the CU count (up2_trip_major).
UP2_TRIP = (3, 17, 512, 512, 4, 4, 2, 1, 2, 2, 1)


def up2_trip_major(cus):
    """Fewest planes of [., 512, 512] -> [., 1024, 1024] with more 2 x 4 blocks (256 x 512 a plane) than 32 * cus * 256."""
    return 32 * cus * 256 // (256 * 512) + 1


OUT_SIZE = {
    ROWMARCH[0]: (7, 70), ROWMARCH[1]: (7, 118), ROWMARCH[2]: (4, 199), ROWMARCH[3]: (9, 105), ROWMARCH[4]: (4, 299),
    ROWMARCH[5]: (8, 64), ROWMARCH_TALL: (64, 64),
    RING[0]: (11, 256), RING[1]: (10, 256), RING[2]: (12, 260), RING_REFUSED: (11, 255),
    PLANETILE[0]: (1, 1), PLANETILE[1]: (10, 10), PLANETILE[2]: (1, 300), PLANETILE[3]: (256, 47), PLANETILE[4]: (3, 5),
    PLANETILE[5]: (7, 61), PLANETILE_OVER: (239, 49), PLANETILE_STRIDED: (9, 9),
    UP2[0]: (14, 18), UP2[1]: (10, 5), UP2[2]: (16, 66), UP2[3]: (11, 19), UP2[4]: (14, 18), UP2_TRIP: (1024, 1024),
}

ALL_ROWS = (ROWMARCH + [ROWMARCH_TALL] + RING + [RING_REFUSED] + PLANETILE + [PLANETILE_OVER, PLANETILE_STRIDED] + UP2 +
            [UP2_TRIP])

# The fused blur (fmgan_blur_noise_bias_act_f32) with unequal pads: the first two ring rows, the first row-march row and the
# cropping plane-tile row.
FUSED = [RING[0], RING[1], ROWMARCH[0], PLANETILE[1]]


def row_id(row):
    k, major, in_h, in_w, kh, kw, up, px0, px1, py0, py1 = row
    return f'k{k}-{major}x{in_h}x{in_w}-{kh}x{kw}-up{up}-pad{px0},{px1},{py0},{py1}'
