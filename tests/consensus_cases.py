"""Cases for the device consensus (csrc/consensus.hip) that are built to take a named path, and
a classifier that says which path a frame takes, from real CPython sets.

lookup_order_kernel writes a frame's list(consensus & frame_set) in one of four ways:

    asc           every result key is below the result's final table size: ascending
    cons_iter     the frame has more keys than the consensus: the consensus is iterated in its
                  own order, then the result table R is replayed
    frame_asc     the frame has no more keys than the consensus and its own set is ascending:
                  its bits are staged, then R is replayed
    frame_replay  the frame's own set is not ascending: its table S is replayed first, then R

(a frame without a consensus key is ``empty``).  R and S live in LDS or in the per-frame global
scratch by cap = table_size(nc): both in LDS up to 512 (nc <= 306), S in scratch at 2048
(nc 307 ... 1228), both in scratch at 8192 (nc >= 1229).  vote_key_kernel replays a template's
first frame when that frame's set is not ascending.

classify(sets, n_kp_global) restates these selections with set / Counter; path_case builds
frames of every kind around a pool of templates that wins the vote; size_edge_case and
word_edge_case put frame and template counts on the kernels' chunk, pass, block and word
edges.  tests/test_consensus_cases_host.py holds (without a GPU) what the cases must reach,
tests/test_gpu_consensus_paths.py runs them on the device.  Not collected by pytest; importing
it needs no GPU.

What classify reports for PATH_SHAPES at PATH_SEED (frames per path; the largest R and S a
frame builds; in every case the consensus is the pool):

    (n_tpl, nc, F)      empty  asc  cons_iter  frame_asc  frame_replay   cap  R max  S max
    (600, 100, 64)         11    7         14          7            25   512    512    512
    (4096, 500, 64)        13    7         14          7            23  2048   2048   2048
    (10000, 1300, 48)       8    5         12          5            18  8192   8192   8192
    (2100, 306, 24)         3    2          6          3            10   512    512    512
    (2100, 307, 24)         2    2          6          3            11  2048   2048   2048
    (10000, 1228, 24)       3    2          6          3            10  2048   2048   2048
    (10000, 1229, 24)       4    2          6          3             9  8192   8192   8192
"""
from collections import Counter
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

import oracle

PATHS = ("empty", "asc", "cons_iter", "frame_asc", "frame_replay")
REPLAYED = ("cons_iter", "frame_asc", "frame_replay")  # the paths that build R

# (n_tpl, n_kp_global, F): three sizes of set table, then both sides of the two thresholds
PATH_SHAPES = ((600, 100, 64), (4096, 500, 64), (10000, 1300, 48),
               (2100, 306, 24), (2100, 307, 24), (10000, 1228, 24), (10000, 1229, 24))
PATH_SEED = 1
EDGE_N_TPL = 160
EDGE_F = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049)
WORD_N_TPL = (31, 32, 33, 63, 64, 65, 255, 256, 257)
WORD_F = 20


def table_size(m: int) -> int:
    """pyset_table_size: the table of a set after m insertions of distinct keys into an empty
    set (Objects/setobject.c: resize at fill * 5 >= mask * 3 to the smallest power of two above
    4 * used, 2 * used beyond 50000)."""
    mask = 7
    while True:
        u = (3 * mask + 4) // 5
        if m < u:
            return mask + 1
        minused = u * 2 if u > 50000 else u * 4
        ns = 8
        while ns <= minused:
            ns <<= 1
        mask = ns - 1


def scratch_words(cap: int) -> int:
    """Per-frame words of global scratch the lookup needs: 2 cap for each table not in LDS."""
    return 0 if cap <= 512 else 2 * cap if cap <= 2048 else 4 * cap


def bits(sets, n_tpl: int) -> np.ndarray:
    """[F, ceil(n_tpl / 32)] u32 survivor bitmasks; the unused bits of the last word are zero."""
    kb = np.zeros((len(sets), (n_tpl + 31) // 32), np.uint32)
    for f, s in enumerate(sets):
        k = np.fromiter(s, np.int64, len(s))
        np.bitwise_or.at(kb[f], k >> 5, (np.uint32(1) << (k & 31).astype(np.uint32)))
    return kb


def as_set(keys) -> Set[int]:
    """A frame's set, built from its ascending key list as the pipeline does (VA:214)."""
    return set(sorted(int(k) for k in keys))


def is_ascending(s: Set[int]) -> bool:
    return not s or max(s) < table_size(len(s))


@dataclass
class Classes:
    nc: int
    cap: int
    path: List[str]                 # per frame
    r_size: List[int]               # per frame: table_size(len(result))
    s_size: List[int]               # per frame: table_size(len(frame))
    first: Dict[int, int]           # per voted template: its first frame
    first_replayed: Dict[int, bool]  # ... and whether that frame's set must be replayed

    def counts(self) -> Dict[str, int]:
        c = Counter(self.path)
        return {p: c[p] for p in PATHS}

    def frames(self, path: str) -> List[int]:
        return [f for f, p in enumerate(self.path) if p == path]

    def r_max(self) -> int:
        """The largest R a frame really builds."""
        return max([r for p, r in zip(self.path, self.r_size) if p in REPLAYED], default=0)

    def s_max(self) -> int:
        """The largest S a frame really builds."""
        return max([s for p, s in zip(self.path, self.s_size) if p == "frame_replay"], default=0)


def classify(sets, n_kp_global: int, cons: Optional[Set[int]] = None) -> Classes:
    """The device's path selection per frame and the vote kernel's queue per template.  ``cons``
    is the consensus of these frames unless given (a frame range of a larger job)."""
    if cons is None:
        cons = oracle.consensus(sets, n_kp_global, 1)[0]
    nc = len(cons)
    path, r_size, s_size = [], [], []
    first: Dict[int, int] = {}
    for f, s in enumerate(sets):
        res = cons & s
        m, flen = len(res), len(s)
        r_size.append(table_size(m))
        s_size.append(table_size(flen))
        if m == 0:
            path.append("empty")
        elif max(res) < table_size(m):
            path.append("asc")
        elif flen > nc:
            path.append("cons_iter")
        elif is_ascending(s):
            path.append("frame_asc")
        else:
            path.append("frame_replay")
        for k in s:
            first.setdefault(k, f)
    replayed = {k: not is_ascending(sets[f]) for k, f in first.items()}
    return Classes(nc, table_size(nc), path, r_size, s_size, first, replayed)


@dataclass
class Case:
    name: str
    n_tpl: int
    n_kp_global: int
    sets: List[Set[int]]
    pool: Optional[Set[int]] = None
    _ref: dict = field(default_factory=dict, repr=False)

    @property
    def F(self) -> int:
        return len(self.sets)

    @property
    def kb(self) -> np.ndarray:
        if "kb" not in self._ref:
            self._ref["kb"] = bits(self.sets, self.n_tpl)
            self._ref["kb"].setflags(write=False)
        return self._ref["kb"]

    @property
    def counter(self) -> Counter:
        """Counter([x for s in kp_idxs_list for x in s]) (VA:239)."""
        if "counter" not in self._ref:
            self._ref["counter"] = Counter([x for s in self.sets for x in s])
        return self._ref["counter"]

    @property
    def consensus(self) -> Tuple[Set[int], tuple, tuple]:
        """oracle.consensus: (set, most_common order, counts)."""
        if "cons" not in self._ref:
            self._ref["cons"] = oracle.consensus(self.sets, self.n_kp_global, 1)
        return self._ref["cons"]

    @property
    def lists(self) -> List[List[int]]:
        """oracle.lookup: every frame's list(consensus & frame_set)."""
        if "lists" not in self._ref:
            self._ref["lists"] = oracle.lookup(self.consensus[0], self.sets)
        return self._ref["lists"]

    @property
    def classes(self) -> Classes:
        if "classes" not in self._ref:
            self._ref["classes"] = classify(self.sets, self.n_kp_global, self.consensus[0])
        return self._ref["classes"]


def csr(lists) -> Tuple[np.ndarray, np.ndarray]:
    """pt_off [F + 1] and pt_idx of per-frame lists."""
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    idx = np.fromiter((k for x in lists for k in x), np.int32, int(off[-1]))
    return off, idx


# ------------------------------------------------------------------ lookup paths
def path_case(n_tpl: int, n_kp_global: int, F: int, seed: int = PATH_SEED) -> Case:
    """Frames of nine kinds, in turn, around a pool of n_kp_global templates that every third
    frame or so holds whole, so that the pool is the consensus."""
    rng = np.random.default_rng(seed)
    nc = n_kp_global
    fixed = [0, 1, 2, 3, 4, n_tpl - 1]
    rest = rng.choice(np.arange(5, n_tpl - 1), nc - len(fixed), replace=False)
    pool = np.sort(np.concatenate([fixed, rest])).astype(np.int64)
    strangers = np.setdiff1d(np.arange(n_tpl), pool)
    # the longest run of the pool's smallest keys that sits below its own table size
    n_asc = max(j for j in range(1, nc + 1) if pool[j - 1] < table_size(j))
    # the frame-asc bound, and the pool's largest key below it: it keeps the result off `asc`
    k_fa = max(nc // 3, 1)
    bound = min(table_size(k_fa), n_tpl)
    p_top = int(pool[pool < bound].max())

    def some(a, lo, hi):
        return rng.choice(a, int(rng.integers(lo, hi + 1)), replace=False)

    sets = []
    for f in range(F):
        kind = f % 9
        if kind == 0:    # flen == nc: the frame-set side of flen > nc, S and R of cap entries
            keys = pool
        elif kind == 1:  # flen > nc with the whole result
            keys = np.concatenate([pool, some(strangers, 1, 5)])
        elif kind == 2:  # cons-iter with m < nc
            keys = np.concatenate([some(pool, nc // 4, 3 * nc // 4), rng.choice(strangers, nc + 50, replace=False)])
        elif kind == 3:  # frame-asc: an ascending frame whose result is not
            keys = np.union1d(rng.choice(bound, k_fa, replace=False)[: k_fa - 1], [p_top])
        elif kind == 4:  # frame-replay
            keys = some(pool, max(nc // 4, 1), nc)
        elif kind == 5:  # flen == nc - 1
            keys = np.delete(pool, int(rng.integers(0, nc)))
        elif kind == 6:
            keys = []
        elif kind == 7:
            keys = some(np.arange(n_tpl), 1, 5)
        else:            # asc
            keys = pool[:n_asc]
        sets.append(as_set(keys))
    return Case(f"path-{n_tpl}-{n_kp_global}-{F}", n_tpl, n_kp_global, sets, pool=set(pool.tolist()))


# ------------------------------------------------------------------ frame-count edges
# templates that only one frame holds: the chunk edges of vote_count_kernel (64 frames) and the
# last frame
def _only_at(F: int) -> Dict[int, int]:
    at: Dict[int, int] = {}
    for f, t in ((63, 150), (64, 151), (65, 152), (127, 153), (128, 154), (F - 1, 155)):
        if 0 <= f < F:
            at.setdefault(f, t)
    return at


def size_edge_case(F: int, seed: int = 0) -> Case:
    """Dense random frames over templates 0 ... 149 of EDGE_N_TPL.  Before every multiple b of 16
    (lookup_scan_kernel's lane share; 64 and 1024 are its wave and pass) frame b - 1 holds a
    single key and frame b + 1 none, or one of the templates of _only_at; frame b stays dense,
    so the counts on the two sides of b differ and none is zero.  n_kp_global = n_tpl: every
    voted template is in the consensus and a frame's count is its size."""
    rng = np.random.default_rng(1000 + F + seed)
    n_tpl = EDGE_N_TPL
    on = rng.random((F, 150)) < 0.5
    only = _only_at(F)
    sets = []
    for f in range(F):
        if (f + 1) % 16 == 0:
            keys = [only.get(f, 0)]
        elif f % 16 == 1 and f > 16:
            keys = [only[f]] if f in only else []
        else:
            keys = np.flatnonzero(on[f]).tolist() + [0, 1] + ([only[f]] if f in only else [])
        sets.append(as_set(keys))
    return Case(f"frames-{F}", n_tpl, n_tpl, sets)


def edge_boundaries(F: int) -> List[int]:
    return list(range(16, F, 16))


# ------------------------------------------------------------------ template-count edges
def word_edge_case(n_tpl: int, seed: int = 0) -> Case:
    """n_tpl on the edges of a bitmask word (32) and of a vote_count_kernel block (256): random
    frames, template n_tpl - 1 in two of them."""
    rng = np.random.default_rng(2000 + n_tpl + seed)
    keys = [np.flatnonzero(rng.random(n_tpl - 1) < 0.4).tolist() for _ in range(WORD_F)]
    keys[3].append(n_tpl - 1)
    keys[WORD_F - 1].append(n_tpl - 1)
    keys[7] = []
    sets = [as_set(k) for k in keys]
    return Case(f"templates-{n_tpl}", n_tpl, max(n_tpl // 2, 1), sets)


_CACHE: Dict[tuple, Case] = {}


def _cached(key, make) -> Case:
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def get_path_case(shape) -> Case:
    return _cached(("path",) + tuple(shape), lambda: path_case(*shape))


def get_size_edge_case(F: int) -> Case:
    return _cached(("frames", F), lambda: size_edge_case(F))


def get_word_edge_case(n_tpl: int) -> Case:
    return _cached(("templates", n_tpl), lambda: word_edge_case(n_tpl))


def all_cases() -> List[Case]:
    return ([get_path_case(s) for s in PATH_SHAPES] + [get_size_edge_case(F) for F in EDGE_F]
            + [get_word_edge_case(n) for n in WORD_N_TPL])
