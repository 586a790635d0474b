"""Host model of leaf symmetries (hz_leaf_sym_keys, hz_mcts_set_leaf_symmetry,
BatchedMCTS.search(leaf_symmetry=)), and the two evaluators its tests need.  A
helper, not a test.

LeafSymModel is tests/mcts_carry_model.py's CarryModel whose search passes the
leaf's node id to the evaluation.  With a key it restates the rule of
include/hz_abi.h ("leaf symmetries"): g = mix64(key ^ (0x9FB21C651E98DF25 *
(node + 1))) >> 62 in Python integers, the evaluator sees
hzamd.symmetry.transform_states' image of the leaf, and the prior of action a
is the image's policy at ACTION_PERM[g][a].  Without a key, and with evaluator
0 / 1, it is CarryModel, i.e. oracle.mcts_search
(tests/test_mcts_leafsym_cpu.py).

Both parity stubs key on plane sums, which no board symmetry changes: under
them a search would pass even if the encoder ignored g.  Hence:

  the cell stub   K = _stub_key + sum rint(3 board[c, y, x]) W[c, y, x] mod 2^31,
                  W = ((index + 1) 2654435761) mod 2^20 over the flat [38, 5, 7]
                  index; policy and value from K by stub_evaluator's formulas.
                  Encoded entries are exactly 0, 1/3, 2/3 or 1, so this is
                  integer arithmetic: the same bits on the host (over
                  oracle.encode) and on the device (a device-row, capturable,
                  row-independent evaluator).  It tells a position from its
                  images.
  the orbit stub  stub_evaluator with the action index replaced by the
                  smallest member of its orbit under ACTION_PERM: equivariant
                  by construction (its key is blind to g, and its policy is
                  constant on orbits), so a search with keys equals the same
                  search without."""
import numpy as np
import torch

import oracle
from hzamd.state import pack_ref, unpack_ref, words_to_array
from hzamd.symmetry import ACTION_PERM, transform_states
from mcts_carry_model import CarryModel, game_over

M64 = (1 << 64) - 1
LEAF_SALT = 0x9FB21C651E98DF25
KEY_SALT = 0xC2B2AE3D27D4EB4F

# The boards the leaf-symmetry tests share (tests/test_mcts_leafsym_cpu.py shows,
# with this model, that they hold every case the device tests rely on), and the
# key of their draws
FIXTURE = {"base": 5200, "n": 130, "spread": 37, "sims": 24, "cpuct": 1.25, "eps": 0.3}
KEYS = {"seed": 20211, "board_base": 700, "move": 9}
SMALL = 20  # the boards of the one-workgroup path (n <= 32)

PERM = np.array(ACTION_PERM, np.int64)         # [4, 143]
ORBIT_MIN = PERM.min(0)                        # the smallest member of each action's orbit
CELL_W = ((np.arange(38 * 5 * 7, dtype=np.int64) + 1) * 2654435761) % (1 << 20)


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def leaf_sym(key, node):
    """The rule: the symmetry of the leaf `node` of a board with this key."""
    return mix64((int(key) & M64) ^ ((LEAF_SALT * (int(node) + 1)) & M64)) >> 62


def host_keys(n, seed, board_base, move):
    """hz_leaf_sym_keys on the host: a list of n Python integers."""
    out = []
    for b in range(n):
        key = mix64(mix64(mix64(seed ^ 0x6A09E667F3BCC908) ^ ((board_base + b) & M64)) ^ move)
        out.append(mix64(key ^ KEY_SALT))
    return out


def image(st, g):
    """The ref state st under g, through hzamd.symmetry.transform_states."""
    if g == 0:
        return np.asarray(st, np.int16)
    words = torch.from_numpy(words_to_array([pack_ref(st)]))
    return unpack_ref(transform_states(words, int(g))[0].numpy())


# ------------------------------------------------------------------ evaluators
def _host_stub_key(board, glob):
    """hzamd.mcts._stub_key over one oracle.encode result."""
    n0 = int(np.rint(board[0:18].astype(np.float64).sum()))
    n1 = int(np.rint(board[18:36].astype(np.float64).sum()))
    cp = int(np.rint(board[36].max()))
    ph3 = int(np.rint(np.float32(board[37].max()) * np.float32(3.0)))
    pc = np.rint(glob[0:36].astype(np.float64) * 3.0).astype(np.int64)
    w = int((pc * np.arange(1, 37, dtype=np.int64)).sum())
    return (n0 * 73 + n1 * 151 + ph3 * 7 + cp * 3 + w * 13) % (1 << 31)


def _host_from_key(K, index):
    h = (index * 2654435761 + K * 40503) % (1 << 32)
    pol = ((h >> 22) + 1).astype(np.float32) / np.float32(1024.0)
    return pol, float(np.float64((K % 255) - 127) / 128.0)


def cell_key(st):
    """The cell stub's key of a ref state."""
    board, glob = oracle.encode(st)
    cells = int((np.rint(board.astype(np.float64).ravel() * 3.0).astype(np.int64) * CELL_W).sum())
    return (_host_stub_key(board, glob) + cells) % (1 << 31)


def cell_stub_host(st):
    return _host_from_key(cell_key(st), np.arange(143, dtype=np.int64))


def orbit_stub_host(st):
    board, glob = oracle.encode(st)
    return _host_from_key(_host_stub_key(board, glob), ORBIT_MIN)


class _DeviceStub:
    """A stub on the device-row protocol (device integer ops only: capturable;
    every row a function of that row alone)."""
    device_rows = capturable = row_independent = True

    def __init__(self, orbit):
        self.orbit = orbit
        self.graph_key = (self, 0)
        self._t = {}

    def _tables(self, dev):
        if dev not in self._t:
            self._t[dev] = (torch.from_numpy(CELL_W).to(dev), torch.from_numpy(ORBIT_MIN).to(dev))
        return self._t[dev]

    def __call__(self, board, glob, rows=None, count=None):
        from hzamd.mcts import _stub_key
        w, orbit = self._tables(board.device)
        K = _stub_key(board, glob)
        index = orbit
        if not self.orbit:
            cells = (torch.round(board.double().reshape(board.shape[0], -1) * 3.0).long() * w).sum(1)
            K = (K + cells) % (1 << 31)
            index = torch.arange(143, device=board.device, dtype=torch.int64)
        h = (index.unsqueeze(0) * 2654435761 + K.unsqueeze(1) * 40503) % (1 << 32)
        pol = ((h >> 22) + 1).to(torch.float32) / 1024.0
        val = ((K % 255) - 127).to(torch.float64) / 128.0
        return pol, val.to(torch.float32)


CELL_STUB = _DeviceStub(orbit=False)
ORBIT_STUB = _DeviceStub(orbit=True)
HOST_STUBS = {"cell": cell_stub_host, "orbit": orbit_stub_host}


# ----------------------------------------------------------------------- model
class LeafSymModel(CarryModel):
    """One board under search(leaf_symmetry=).  evaluator: 0 / 1 (the oracle's
    stubs), "cell" or "orbit"; key: the board's key (None: the gate is off).
    evaluated: (node, g, leaf state) of every evaluation, in order."""

    def __init__(self, ref_state, mt, evaluator=0, key=None, **kw):
        named = evaluator in HOST_STUBS
        super().__init__(ref_state, mt, 0 if named else evaluator, **kw)
        if named:
            self.eval = HOST_STUBS[evaluator]
        self.key = key
        self.evaluated = []

    def evaluate(self, st, node):
        g = 0 if self.key is None else leaf_sym(self.key, node)
        self.evaluated.append((node, g, st))
        pol, value = self.eval(image(st, g))
        return np.asarray(pol, np.float32)[PERM[g]].copy(), value

    def search(self, sims, cpuct, noise=None, eps=0.25, noisy=False, max_depth=None):
        """CarryModel.search with the leaf's node id passed to the evaluation."""
        from mcts_carry_model import mix
        E = self.E
        self.first_edge = None
        for _ in range(int(sims)):
            node, path = 0, []
            while self.ne[node] > 0:
                if max_depth is not None and len(path) >= max_depth:
                    self.flag = 1
                    break
                sel = self._select(node, cpuct)
                if node == 0 and self.first_edge is None:
                    self.first_edge = sel - self.e0[0]
                path.append(sel)
                node = int(E["child"][sel])
            st = self.state[node]
            player = int(st[72])
            if game_over(st):
                outcome = 1 if st[75] == 0 else -1 if st[75] == 1 else 0
                value = float(outcome if player == 0 else -outcome) if outcome else 0.0
            else:
                pol, value = self.evaluate(st, node)
                legal = np.flatnonzero(oracle.legal(st))
                if node == 0 and noisy and noise is not None:
                    for i, a in enumerate(legal):
                        pol[a] = mix(pol[a], eps, noise[i])
                if len(legal) and self.ne[node] == 0:
                    self._expand(node, st, legal, pol, player)
            for e in path:
                E["n"][e] += 1
                E["w"][e] = E["w"][e] + float(value) * (1.0 if E["player"][e] == player else -1.0)
