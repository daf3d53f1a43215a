"""Collision filters in numpy (include/physics_hip.h): the rule the narrow phase applies, and the
encoding of a filter in the spare words of a 96-byte halo record. For callers that precompute or inspect what may touch
what, and for the tests; the library applies the rule on the device itself."""
import numpy as np

from ._abi import FILTER_DEFAULT_CATEGORY, FILTER_DEFAULT_MASK

DEFAULT_WORD = FILTER_DEFAULT_CATEGORY | (FILTER_DEFAULT_MASK << 16)  # category | mask << 16 of the default filter


def collide(cat_a, mask_a, group_a, cat_b, mask_b, group_b):
    """Whether A and B may form a contact manifold (broadcasting arrays): the same nonzero group decides by its sign,
    anything else needs each category in the other's mask."""
    ca, ma, ga = (np.asarray(x).astype(np.int64) for x in (cat_a, mask_a, group_a))
    cb, mb, gb = (np.asarray(x).astype(np.int64) for x in (cat_b, mask_b, group_b))
    same = (ga == gb) & (ga != 0)
    return np.where(same, ga > 0, ((ca & mb) != 0) & ((cb & ma) != 0))


def halo_encode(category, mask, group, full_inertia=False):
    """(q[4].w, q[5].w) as u32 bits of a body record: the full-inertia flag in bit 0 and the group in bits 16-31 of the
    first, (category | mask << 16) ^ DEFAULT_WORD in the second, so the default filter encodes as (flag, 0)."""
    c = np.asarray(category).astype(np.uint32)
    m = np.asarray(mask).astype(np.uint32)
    g = np.asarray(group).astype(np.int16).view(np.uint16).astype(np.uint32)
    q4w = np.asarray(full_inertia).astype(np.uint32) | (g << np.uint32(16))
    q5w = (c | (m << np.uint32(16))) ^ np.uint32(DEFAULT_WORD)
    return q4w, q5w


def halo_decode(q4w, q5w):
    """(category u16, mask u16, group i16, full-inertia flag) from the two record words."""
    q4w = np.asarray(q4w).astype(np.uint32)
    word = np.asarray(q5w).astype(np.uint32) ^ np.uint32(DEFAULT_WORD)
    group = (q4w >> np.uint32(16)).astype(np.uint16).view(np.int16)
    return (word & np.uint32(0xFFFF)).astype(np.uint16), (word >> np.uint32(16)).astype(np.uint16), group, (q4w & np.uint32(1)) != 0
