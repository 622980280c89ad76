"""
Plain-Python model of zk_lookup_find / zk_lookup3_find: the first occurrence of every row's value in the table, by dictionary, and the
count and the first row of the misses.  A key is the tuple of all limbs of an entry (four for one column, twelve for a triple).
"""
import numpy as np

import pyoracle as po

_R = (1 << 256) % po.R_MOD
ONE = tuple((_R >> (64 * i)) & (2**64 - 1) for i in range(4))  # the limbs of the Montgomery form of 1


def keys(cols):
    """one [N, 4] array, or a sequence of them (the columns of a triple) -> N tuples of python ints"""
    if isinstance(cols, np.ndarray) and cols.ndim == 2:
        cols = [cols]
    rows = np.concatenate([np.asarray(c, dtype=np.uint64).reshape(-1, 4) for c in cols], axis=1)
    return [tuple(int(v) for v in r) for r in rows]


def find(t, f, qk=None):
    """-> (idx, bad, first): idx[x] = the smallest y with t[y] == f[x] for a selected row that is in the table, else 0; bad = how many rows
    are selected and not in the table, or carry a qk that is neither 0 nor 1; first = the smallest such row (None: none).  qk None: every
    row is selected"""
    tk, fk = keys(t), keys(f)
    first_of = {}
    for y, k in enumerate(tk):
        if k not in first_of:
            first_of[k] = y
    q = [ONE] * len(fk) if qk is None else keys(qk)
    idx, bad_rows = [0] * len(fk), []
    for x, k in enumerate(fk):
        if q[x] == (0, 0, 0, 0):
            continue
        if q[x] != ONE or k not in first_of:
            bad_rows.append(x)
            continue
        idx[x] = first_of[k]
    return idx, len(bad_rows), (bad_rows[0] if bad_rows else None)


def multiplicities(idx, qk=None):
    """m[y] = #{x selected : idx[x] = y} as python ints"""
    q = [ONE] * len(idx) if qk is None else keys(qk)
    m = [0] * len(idx)
    for x, y in enumerate(idx):
        if q[x] == ONE:
            m[y] += 1
    return m
