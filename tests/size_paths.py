"""Case lists of tests/test_gpu_size_paths.py and the host-side rules by which the library picks a kernel path from the image
size, restated so that tests/test_host_logic.py can check without a GPU that the cases reach every path."""

# (Hp, Wp): 480p <8>; 1080p <20>; the <20>/<40> and the <40>/tall boundaries on narrow images; portrait 1080p <40>; the two
# 4K orientations (<40>, tall)
EDT_SIZES = [(480, 832), (1088, 1920), (1280, 64), (1296, 64), (1920, 1088), (2560, 64), (2592, 64), (2176, 3840), (3840, 2176)]
EDT_PATTERNS = ["blobs", "corner", "column_row", "sparse", "lattice_31_32", "lattice_33_64", "ties", "band", "empty"]
EDT_PATTERNS_4K = ["corner", "sparse", "band"]
EDT_CASES = [(hp, wp, pat) for hp, wp in EDT_SIZES for pat in (EDT_PATTERNS_4K if hp * wp > 4_000_000 else EDT_PATTERNS)]

# (hw, T): 480p (30 x 52) and 1080p (68 x 120) with 2, 3, 5 slots; 480p with 9 and 17 slots (several 8-slot launches); 4K
MR_SHAPES = [(1560, 2), (1560, 3), (1560, 5), (8160, 2), (8160, 3), (8160, 5), (1560, 9), (1560, 17), (32640, 3)]


def edt_column_path(Hp):
    """otvm_trimap_encode (edt.hip): the column pass is chosen by len = ceil(Hp / EDT_SEGS), EDT_SEGS = 64."""
    n = -(-Hp // 64)
    return "8" if n <= 8 else "20" if n <= 20 else "40" if n <= 40 else "tall"


def mr_launches(T, hw):
    """mr_chunks / mr_launch_partials (memory_read_f16x3.hip): one launch per 8 slots; its memory axis of n * ceil(hw / 64)
    tiles is cut into chunks of chunk_tiles tiles (ceil(512 / query blocks) chunks at most); 'crossing' counts the chunks
    that span a slot boundary (the t == tiles_per_slot wrap inside the kernel)."""
    tps = -(-hw // 64)
    out = []
    for s0 in range(0, T, 8):
        n = min(8, T - s0)
        total = n * tps
        chunks = min(max(-(-512 // tps), 1), total)
        ct = -(-total // chunks)
        used = -(-total // ct)
        crossing = sum(1 for c in range(used) if (c * ct) // tps != (min(total, (c + 1) * ct) - 1) // tps)
        out.append(dict(chunks=chunks, chunk_tiles=ct, used=used, crossing=crossing))
    return out
