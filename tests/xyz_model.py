"""The cinema colour transform of j2k_hip_params.rgb_to_xyz in numpy, exactly as include/j2k_hip.h defines it: source code ->
linear light by table, the scaled R G B -> X Y Z matrix with every product and sum rounded to binary32, the code as the number
of thresholds <= the value.  The tables can be given in (the library's own: api.xyz_tables) or made from the formula here."""
import numpy as np

M_SRGB_D65 = np.array([[0.4124564, 0.3575761, 0.1804375],
                       [0.2126729, 0.7151522, 0.0721750],
                       [0.0193339, 0.1191920, 0.9503041]], dtype=np.float64)


def eotf(source: int, x: np.ndarray) -> np.ndarray:
    """Code in 0..1 (float64) -> linear light (float64)."""
    x = np.asarray(x, dtype=np.float64)
    if source == 1:
        return np.where(x <= 0.04045, x / 12.92, np.power((x + 0.055) / 1.055, 2.4))
    if source == 2:
        return np.power(x, 2.4)
    if source == 3:
        return x
    raise ValueError(source)


def formula_tables(source: int, src_depth: int, dst_depth: int):
    """(lin, thr, matrix) from the definition: float32 arrays of 2^src_depth, 2^dst_depth - 1 and 3 x 3 values."""
    v = np.arange(1 << src_depth, dtype=np.float64)
    lin = eotf(source, v / float((1 << src_depth) - 1)).astype(np.float32)
    top = (1 << dst_depth) - 1
    c = np.arange(1, top + 1, dtype=np.float64)
    thr = np.power((c - 0.5) / float(top), 2.6).astype(np.float32)
    m = (M_SRGB_D65 * (48.0 / 52.37)).astype(np.float32)
    return lin, thr, m


def promote16(v: np.ndarray) -> np.ndarray:
    """The After Effects 15+1 -> 16 bit Promote of include/j2k_hip.h (wraps to 16 bits)."""
    v = np.asarray(v, dtype=np.uint32)
    return np.where(v > 16384, ((v - 1) << 1) + 1, v << 1) & 0xffff


def quantise_float(x: np.ndarray, depth: int, promote: bool = False) -> np.ndarray:
    """j2k_hip_plane's rule for a float sample: the integer of `depth` bits it stands for."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(x > 1, np.float32(1), np.where(x > 0, x, np.float32(0))).astype(np.float32)
    if promote:
        return promote16((t * np.float32(32768.0) + np.float32(0.5)).astype(np.uint32))
    return (t * np.float32((1 << depth) - 1) + np.float32(0.5)).astype(np.uint32)


def codes(rgb, source: int, src_depth: int, dst_depth: int, tables=None) -> np.ndarray:
    """rgb: (3, ...) integer samples of src_depth bits (after Promote / the float rule) -> (3, ...) X'Y'Z' codes of dst_depth
    bits (int64).  src_depth may be a triple: one depth per channel, with tables = ((lin_r, lin_g, lin_b), thr, m) then."""
    depths = (src_depth,) * 3 if np.isscalar(src_depth) else tuple(src_depth)
    if tables is None:
        lins = [formula_tables(source, d, dst_depth)[0] for d in depths]
        _, thr, m = formula_tables(source, depths[0], dst_depth)
    else:
        lins, thr, m = tables
        if isinstance(lins, np.ndarray):
            lins = [lins] * 3
    m = np.asarray(m, dtype=np.float32).reshape(3, 3)
    rgb = [np.minimum(np.asarray(rgb[c]).astype(np.int64), (1 << depths[c]) - 1) for c in range(3)]
    l = [np.asarray(lins[c], dtype=np.float32)[rgb[c]] for c in range(3)]
    out = []
    for i in range(3):
        p = [(m[i, j] * l[j]).astype(np.float32) for j in range(3)]          # every product rounded to binary32
        x = ((p[0] + p[1]).astype(np.float32) + p[2]).astype(np.float32)     # every sum too, left to right
        out.append(np.searchsorted(np.asarray(thr, dtype=np.float32), x, side="right").astype(np.int64))
    return np.stack(out)


def rct(c: np.ndarray) -> np.ndarray:
    """The reversible colour transform of DC-shifted integer components (3, ...)."""
    r, g, b = (np.asarray(c[i], dtype=np.int64) for i in range(3))
    return np.stack([(r + 2 * g + b) >> 2, b - g, r - g])
