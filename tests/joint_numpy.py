"""The joint hazard restated in plain NumPy (tests/test_joint.py): the definitions of the header's "joint hazard (co-exceedance
between sites)" section, written without any of the package's code.  Plain comparisons into a boolean [level][row][unit] array
(the mapped mode in a loop with |=), words built by shifting, counts as an integer matrix product per level."""
import numpy as np


def _levels(levels, n_row):
    lev = np.asarray(levels, dtype=np.float64)
    return np.broadcast_to(lev, (n_row, lev.shape[-1])) if lev.ndim == 1 else lev


def exceed(plane, levels, unit_of=None, n_unit=None):
    """bool [n_level][n_row][n_unit]: unit u of row r reaches level l."""
    plane = np.asarray(plane, dtype=np.float64)
    n_row, n_col = plane.shape
    lev = _levels(levels, n_row)
    with np.errstate(invalid='ignore'):
        hit = plane[None, :, :] >= lev.T[:, :, None]              # [level][row][col]
    if unit_of is None:
        return hit
    unit_of = np.asarray(unit_of)
    n_unit = int(n_unit if n_unit is not None else unit_of.max() + 1)
    out = np.zeros((lev.shape[1], n_row, n_unit), bool)
    for c in range(n_col):
        out[:, :, unit_of[c]] |= hit[:, :, c]
    return out


def words(E):
    """uint64 [..][ceil(n_unit / 64)] of bool [..][n_unit]: bit u & 63 of word u >> 6 is unit u."""
    n_unit = E.shape[-1]
    out = np.zeros(E.shape[:-1] + ((n_unit + 63) // 64,), np.uint64)
    for u in range(n_unit):
        out[..., u >> 6] |= E[..., u].astype(np.uint64) << np.uint64(u & 63)
    return out


def pack_bits(plane, levels, unit_of=None, n_unit=None, engine=None, device=0):
    """(bits [n_level][n_row][n_word] uint64, n_set [n_level][n_row] int32)."""
    E = exceed(plane, levels, unit_of, n_unit)
    return words(E), E.sum(axis=2).astype(np.int32)


def unpack(bits, n_unit):
    """bool [..][n_unit] of uint64 [..][n_word]."""
    bits = np.asarray(bits).view(np.uint64) if np.asarray(bits).dtype == np.int64 else np.asarray(bits, dtype=np.uint64)
    u = np.arange(n_unit)
    return ((bits[..., u >> 6] >> (u & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def cross_from_bool(Ea, Eb):
    """int32 [n_level][n_a][n_b]: E_a @ E_b.T per level, in int64."""
    return np.stack([Ea[l].astype(np.int64) @ Eb[l].astype(np.int64).T for l in range(Ea.shape[0])]).astype(np.int32)


def cross_counts(bits_a, bits_b=None, engine=None, device=0):
    bits_b = bits_a if bits_b is None else bits_b
    n_unit = 64 * np.asarray(bits_a).shape[-1]
    return cross_from_bool(unpack(bits_a, n_unit), unpack(bits_b, n_unit))


def joint(plane, levels, anchors=None, unit_of=None, n_unit=None):
    """(joint [n_level][n_a][n_row] int32, n_set [n_level][n_row] int32) of a whole plane, without bits."""
    E = exceed(plane, levels, unit_of, n_unit)
    a = np.arange(E.shape[1]) if anchors is None else np.asarray(anchors)
    return cross_from_bool(E[:, a], E), E.sum(axis=2).astype(np.int32)
