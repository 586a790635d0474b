"""The board's symmetry group on states, actions, visit rows and records.

The 23-cell board has four automorphisms (the identity, the half turn and two
reflections), and each is an automorphism of the whole game: the rule is
stated in include/hz_abi.h ("board symmetries").  Group element g in 0..3
maps an axial coordinate

    0: (q, r)    1: (-q, -r)    2: (q + r, -r)    3: (-q - r, r)

and a after b is a ^ b, so every element is its own inverse.  CELL_PERM[g][c]
is the index of the image of cell c (cells indexed into sorted(VALID_HEXES)),
ACTION_PERM[g][a] the image of action a.  The tables are built here from the
coordinate maps; csrc/hz_sym.hpp builds the device form from the same maps.

The torch forms run on any device; transform_records on a CUDA tensor is the
HIP kernel (hz_sym_records), bit-identical to the torch form.
"""
import torch

from . import distributed as hd
from .state import CELL_OF, SORTED_COORDS

N_SYM = 4
N_CELLS = 23
N_ACTIONS = 143

_MAPS = (
    lambda q, r: (q, r),
    lambda q, r: (-q, -r),
    lambda q, r: (q + r, -r),
    lambda q, r: (-q - r, r),
)

CELL_PERM = tuple(tuple(CELL_OF[f(q, r)] for (q, r) in SORTED_COORDS) for f in _MAPS)


def transform_action(a, g):
    """Action a under g: pile choices (a < 5) are kept, the placement
    5 + 23 t + c goes to 5 + 23 t + CELL_PERM[g][c]."""
    a = int(a)
    if a < 5:
        return a
    t, c = divmod(a - 5, N_CELLS)
    return 5 + N_CELLS * t + CELL_PERM[g & 3][c]


ACTION_PERM = tuple(tuple(transform_action(a, g) for a in range(N_ACTIONS)) for g in range(N_SYM))


def compose(a, b):
    """The element that applies b, then a."""
    return (a ^ b) & 3


_tables = {}


def _table(name, device):
    key = (name, str(device))
    if key not in _tables:
        src = CELL_PERM if name == "cell" else ACTION_PERM
        _tables[key] = torch.tensor(src, dtype=torch.int64, device=device)
    return _tables[key]


def _sym_index(g, m, device):
    """g (an int, or a tensor of m elements) -> int64 [m] on device, in 0..3."""
    if torch.is_tensor(g):
        if g.numel() != m:
            raise ValueError(f"{g.numel()} symmetries for {m} items")
        return g.reshape(m).to(device=device, dtype=torch.int64) & 3
    return torch.full((m,), int(g) & 3, dtype=torch.int64, device=device)


def transform_states(states, g):
    """states int64 [M, 6] under g (an int, or [M]): in the four plane words
    the stack-code bit of cell c moves to cell CELL_PERM[g][c] for both
    players (bits 0..22 and 32..54); every other bit, and the piles and misc
    words, are kept."""
    m = states.shape[0]
    dev = states.device
    perm = _table("cell", dev)[_sym_index(g, m, dev)]                 # [M, 23]: destination of cell c
    planes = states[:, :4].to(torch.int64)
    cells = torch.arange(N_CELLS, device=dev, dtype=torch.int64)
    keep = ~(((1 << N_CELLS) - 1) | (((1 << N_CELLS) - 1) << 32))
    out = planes & keep
    for base in (0, 32):
        bits = (planes.unsqueeze(2) >> (cells + base)) & 1            # [M, 4, 23]
        out = out | (bits << (perm.unsqueeze(1) + base)).sum(2)       # distinct bits: the sum is an or
    return torch.cat([out, states[:, 4:].to(torch.int64)], dim=1)


def transform_visits(visits, g):
    """visits [M, 143] (counts or policies, any dtype) under g: the entry of
    action a moves to action ACTION_PERM[g][a]."""
    m = visits.shape[0]
    dev = visits.device
    perm = _table("action", dev)[_sym_index(g, m, dev)]               # [M, 143]
    # the map is an involution: image[a] = source[perm[a]]
    return visits.gather(1, perm)


def _transform_records_torch(records, g):
    states, visits, z, player = hd.unpack_records(records)
    return hd.pack_records(transform_states(states, g), transform_visits(visits, g), z, player)


def transform_records(records, g, out=None):
    """Packed records int64 [M, 42] under g (an int, or a [M] tensor): the
    state words as transform_states, the 143 u16 slots as transform_visits,
    the z and player bytes kept.  A CUDA tensor goes through hz_sym_records
    (out may be the records tensor itself: in place); a CPU tensor through the
    torch form."""
    m = records.shape[0]
    if records.device.type != "cuda":
        res = _transform_records_torch(records, g)
        if out is None:
            return res
        out.copy_(res)
        return out
    from . import _native as nat
    dev = records.device
    rec = records.contiguous()
    if out is None:
        out = torch.empty_like(rec)
    elif out.shape != rec.shape or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int64 tensor of the records' shape on their device")
    sym = _sym_index(g, m, dev).to(torch.uint8)
    if m:
        nat.check(nat.lib().hz_sym_records(nat.ptr(rec), m, nat.ptr(sym), nat.ptr(out), nat.stream_ptr(dev)),
                  "hz_sym_records")
    return out
