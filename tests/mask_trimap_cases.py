"""Sizes and masks of the otvm_trimap_from_mask tests (as tests/size_paths.py for the convs): the sizes the issue names and one
size on each side of every size-selected path listed at the top of otvm_amd/csrc/mask_trimap.hip.  No torch, no GPU."""
import numpy as np

# H x W
BASE_SIZES = [(1, 1), (1, 37), (37, 1), (33, 47), (70, 129), (135, 241)]
# columns, rows per thread: H <= 512 -> 8, <= 1280 -> 20, <= 2560 -> 40, above: one thread per column (narrow images: the path
# depends on H alone).  rows, segments: W <= 1024 one workgroup per row, above several.  rows, stores: W % 4 == 0 -> four pixels
# per store (33x48, 3x1024, 5x1028), otherwise pixel by pixel (33x47, 3x1025).
PATH_SIZES = [(512, 19), (513, 19), (1280, 12), (1281, 12), (2560, 8), (2561, 8),
              (33, 48), (3, 1024), (3, 1025), (5, 1028)]
SIZES = BASE_SIZES + PATH_SIZES
T_VALUES = [0, 1, 2, 8, 25, 400, 65025]
THRESHOLDS = [(127, 128), (25, 230), (0, 255)]
CPU_SIZES = [(1, 1), (1, 37), (37, 1), (33, 47), (40, 61)]
CPU_T_VALUES = [0, 1, 2, 8, 25, 30, 400]


def soft_mask(H, W, seed):
    """A soft mask with structure at several scales: blobs of foreground and background with soft rims, a few isolated pixels."""
    g = np.random.default_rng(seed)
    cell = 7
    coarse = g.random((H // cell + 2, W // cell + 2))
    m = np.kron(coarse, np.ones((cell, cell)))[:H, :W]
    m = np.where(m > 0.62, 255.0, np.where(m < 0.38, 0.0, 255.0 * g.random((H, W))))
    speck = g.random((H, W)) < 0.01
    m[speck] = 255.0 - m[speck]
    return m.astype(np.uint8)


def density_mask(H, W, p, seed):
    """Independent pixels, foreground with probability p (0: empty, 1: full)."""
    return np.where(np.random.default_rng(seed).random((H, W)) < p, 255, 0).astype(np.uint8)


def one_pixel(H, W, inside):
    """All background with one foreground pixel (inside=255) or all foreground with one background pixel (inside=0)."""
    m = np.full((H, W), 255 - inside, np.uint8)
    m[H // 2, W // 3] = inside
    return m


def disc(H, W, cy, cx, radius):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius, 255, 0).astype(np.uint8)
