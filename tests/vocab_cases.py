"""Constructed vocabularies, query descriptors and node-id frames for tests/test_vocab_edges.py.

A tree is a list of (parent, flag, descriptor, weight), one entry per line of the text format (TemplatedVocabulary.h:1337-1420:
node ids count the lines from 1, the root is node 0 and has no line).  `flag` is the isLeaf column exactly as write_text emits
it, so a tree may flag a node that later receives children, or leave a childless node unflagged.  Nothing here looks at the
product; tests/vocab_reference.py says what each tree means."""
import collections

import numpy as np

Tree = collections.namedtuple("Tree", "name k L scoring weighting nodes")
Case = collections.namedtuple("Case", "family tree queries")
FvBatch = collections.namedtuple("FvBatch", "name cap n node")        # n [frames] as passed in d_n, node [frames, cap] u32

POISON = 0xDEADBEEF


def rand_desc(rng, n=None):
    return rng.randint(0, 256, 32 if n is None else (n, 32)).astype(np.uint8)


def flip(desc, *bits):
    """`desc` with the given bits (0 .. 255, bit b = byte b // 8, mask 1 << b % 8) inverted."""
    d = np.array(desc, np.uint8)
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def near(rng, desc, nbits=20):
    return flip(desc, *rng.choice(256, nbits, replace=False))


class Builder:
    """Nodes in the order of the add() calls = file order.  flag None: by structure when the tree is taken; weight None: a positive
    six-decimal weight on childless nodes, 0 on the others."""

    def __init__(self, name, k, L, scoring=0, weighting=0, seed=0):
        self.name, self.k, self.L, self.scoring, self.weighting = name, k, L, scoring, weighting
        self.rng = np.random.RandomState(seed)
        self.rows = []

    def add(self, parent, desc=None, weight=None, flag=None):
        assert 0 <= parent <= len(self.rows)
        self.rows.append([parent, flag, rand_desc(self.rng) if desc is None else np.array(desc, np.uint8), weight])
        return len(self.rows)

    def desc(self, nid):
        return self.rows[nid - 1][2]

    def tree(self):
        has_child = set(r[0] for r in self.rows)
        nodes = []
        for i, (parent, flag, desc, weight) in enumerate(self.rows, 1):
            leaf = i not in has_child
            if weight is None:
                weight = float(np.round(self.rng.uniform(0.5, 12.0), 6)) if leaf else 0.0
            nodes.append((parent, int(leaf if flag is None else flag), desc, float(weight)))
        return Tree(self.name, self.k, self.L, self.scoring, self.weighting, nodes)


def write_text(tree, path, trailing_newline=False):
    lines = ["%d %d %d %d" % (tree.k, tree.L, tree.scoring, tree.weighting)]
    for parent, flag, desc, weight in tree.nodes:
        lines.append("%d %d %s %s" % (parent, flag, " ".join(str(int(b)) for b in desc), repr(float(weight))))
    with open(path, "w") as f:
        f.write("\n".join(lines) + ("\n" if trailing_newline else ""))
    return path


def arrays(tree):
    """(desc [n, 32], weight [n], parent [n], flag [n]) with the root as entry 0, as pilotguru_amd.vocab.pack_vocabulary takes them."""
    n = len(tree.nodes) + 1
    desc, weight = np.zeros((n, 32), np.uint8), np.zeros(n, np.float64)
    parent, flag = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    for i, (p, f, d, w) in enumerate(tree.nodes, 1):
        desc[i], weight[i], parent[i], flag[i] = d, w, p, f
    return desc, weight, parent, flag


def reorder(tree, order, name):
    """The same tree with its lines in another order (`order`: old node ids, every parent before its children)."""
    new_id = {0: 0}
    for new, old in enumerate(order, 1):
        new_id[old] = new
    nodes = []
    for old in order:
        p, f, d, w = tree.nodes[old - 1]
        nodes.append((new_id[p], f, d, w))
    return Tree(name, tree.k, tree.L, tree.scoring, tree.weighting, nodes)


def children_of(tree):
    ch = collections.defaultdict(list)
    for i, (p, _, _, _) in enumerate(tree.nodes, 1):
        ch[p].append(i)
    return ch


def depth_first_order(tree):
    ch, out = children_of(tree), []

    def walk(i):
        for c in ch[i]:
            out.append(c)
            walk(c)
    walk(0)
    return out


def interleaved_order(tree, rng):
    """A random order that keeps parents in front of their children and siblings in their order."""
    ch = children_of(tree)
    ready, out = [0], []                                       # nodes whose next child may be written
    nxt = collections.defaultdict(int)
    while ready:
        p = ready[rng.randint(len(ready))]
        c = ch[p][nxt[p]]
        nxt[p] += 1
        if nxt[p] == len(ch[p]):
            ready.remove(p)
        out.append(c)
        if ch[c]:
            ready.append(c)
    return out


def grow(b, parent, depth, arity, leaf_prob, budget):
    """The recursion order of the reference's create() / HKmeansStep (the children of a node are appended together, then each is
    expanded in turn).  arity(rng, depth) children per node, a child at depth < L stays a leaf with
    probability leaf_prob; budget[0] bounds the number of nodes."""
    rng = b.rng
    kids = []
    for _ in range(arity(rng, depth)):
        if budget[0] <= 0 and kids:
            break
        budget[0] -= 1
        base = b.desc(parent) if parent else rand_desc(rng)
        kids.append(b.add(parent, near(rng, base, 28) if parent else base))
    for c in kids:
        if depth + 1 < b.L and budget[0] > 0 and rng.uniform() >= leaf_prob:
            grow(b, c, depth + 1, arity, leaf_prob, budget)


def node_queries(tree, rng, nrandom=20, nnear=40):
    """Every node's own descriptor (distance 0 somewhere on its path), descriptors near nodes, and random ones."""
    descs = [d for _, _, d, _ in tree.nodes]
    q = list(descs)
    for _ in range(nnear):
        q.append(near(rng, descs[rng.randint(len(descs))], rng.randint(1, 40)))
    q.extend(rand_desc(rng, nrandom))
    return np.array(q, np.uint8)


# ---- the families -------------------------------------------------------------------------------------------------------------

def ragged_tree(name="ragged", seed=1, k=5, L=4, scoring=0, weighting=0, at_least=40):
    """1 .. k children per node, every third inner node with a single child; the first seed from 100 * seed on whose tree has
    `at_least` nodes."""
    for s in range(100 * seed, 100 * seed + 100):
        b = Builder(name, k, L, scoring, weighting, s)
        count = [0]

        def arity(rng, depth):
            count[0] += 1
            return 1 if count[0] % 3 == 0 else rng.randint(1 if depth else 2, k + 1)
        grow(b, 0, 0, arity, 0.2, [400])
        if len(b.rows) >= at_least:
            return b.tree()
    raise AssertionError("no ragged tree of %d nodes" % at_least)


def family_ragged():
    out = []
    for seed in (1, 2):
        t = ragged_tree("ragged%d" % seed, seed)
        out.append(Case("ragged", t, node_queries(t, np.random.RandomState(seed))))
    # a pure chain: one child per node down to depth L, and two words at the bottom
    b = Builder("chain", 3, 5, seed=3)
    p = 0
    for _ in range(4):
        p = b.add(p)
    b.add(p)
    b.add(p)
    t = b.tree()
    out.append(Case("ragged", t, node_queries(t, np.random.RandomState(3), 5, 5)))
    return out


def family_depths():
    """A comb: at every depth d < L a node has a word, an inner node and another word, so words sit at every depth 1 .. L."""
    out = []
    for L in (1, 2, 4, 6):
        b = Builder("comb_L%d" % L, 3, L, seed=10 + L)
        p = 0
        for d in range(1, L + 1):                              # a node's descriptor is near its parent's, so its own descriptor finds it
            base = b.desc(p) if p else rand_desc(b.rng)
            b.add(p, near(b.rng, base, 60))
            mid = b.add(p, near(b.rng, base, 12))
            b.add(p, near(b.rng, base, 60))
            p = mid
        t = b.tree()
        out.append(Case("depths", t, node_queries(t, np.random.RandomState(L), 10, 20)))
    return out


def family_orders():
    t = ragged_tree("order_src", 5)
    rng = np.random.RandomState(5)
    q = node_queries(t, rng)
    out = [Case("orders", reorder(t, depth_first_order(t), "order_depth_first"), q)]
    for i in range(2):
        out.append(Case("orders", reorder(t, interleaved_order(t, rng), "order_interleaved%d" % i), q))
    return out


def family_ties():
    """Every inner node holds [far, x^e1, x^e2, x^e1]: the query x is 1 bit from three siblings at every level, the query x^e1 is at
    distance 0 from two identical siblings at every level; the first of them must win each time."""
    b = Builder("ties", 4, 3, seed=20)
    x = rand_desc(b.rng)
    e1, e2 = 7, 130

    def fill(p, depth):
        b.add(p, near(b.rng, x, 100))
        kids = [b.add(p, flip(x, e1)), b.add(p, flip(x, e2)), b.add(p, flip(x, e1))]
        if depth < b.L:
            for c in kids:
                fill(c, depth + 1)
    fill(0, 1)
    t = b.tree()
    q = [x, flip(x, e1), flip(x, e2), flip(x, e1, e2), flip(x, 200)] + list(rand_desc(b.rng, 10))
    # ties that do not start at the first sibling, and one among all siblings of a node
    b2 = Builder("ties_all_equal", 5, 2, seed=21)
    y = rand_desc(b2.rng)
    for _ in range(5):
        b2.add(0, y)
    for p in range(1, 6):
        for j in range(2 + p % 3):
            b2.add(p, flip(y, 3 * p) if j else flip(y, 3 * p + 1))
    t2 = b2.tree()
    q2 = [y, flip(y, 0), flip(y, 3), flip(y, 4), flip(y, 255)] + list(rand_desc(b2.rng, 5))
    return [Case("ties", t, np.array(q, np.uint8)), Case("ties", t2, np.array(q2, np.uint8))]


def family_last_bits():
    """Siblings that differ only inside byte 31, and queries that equal one of them: only a distance over all 256 bits tells."""
    b = Builder("last_bits", 4, 2, seed=30)
    q = []
    for _ in range(3):
        s = rand_desc(b.rng)
        p = b.add(0, s)
        kids = [near(b.rng, s, 9)]
        kids += [flip(kids[0], *range(248, 256)), flip(kids[0], 255), flip(kids[0], 248)]
        for d in kids:
            b.add(p, d)
        q.extend(kids[1:])
        q.append(flip(s, 255))
    t = b.tree()
    return [Case("last_bits", t, np.array(q, np.uint8))]


def family_flags():
    """The isLeaf column against the structure, both ways: a flagged line that later receives children uses up a word id and is never
    a word; a childless line without the flag ends descents with word 0."""
    out = []
    b = Builder("flags_small", 4, 3, seed=40)
    n1 = b.add(0, weight=1.25, flag=0)                         # childless, unflagged: word 0
    n2 = b.add(0, weight=2.5, flag=1)                          # flagged, then two children: takes word id 0
    b.add(n2, weight=3.5, flag=1)                              # word 1
    b.add(n2, weight=4.5, flag=0)                              # childless, unflagged: word 0
    b.add(0, weight=5.5, flag=1)                               # word 2
    n6 = b.add(0, flag=0)
    b.add(n6, weight=0.75, flag=0)                             # single unflagged child
    t = b.tree()
    out.append(Case("flags", t, node_queries(t, np.random.RandomState(40), 10, 20)))
    # a ragged tree with a tenth of its lines flipped either way
    src = ragged_tree("flags_src", 41)
    rng = np.random.RandomState(41)
    nodes = []
    for p, f, d, w in src.nodes:
        if rng.uniform() < 0.1:
            f, w = 1 - f, (w if w else float(np.round(rng.uniform(0.5, 9.0), 6)))
        nodes.append((p, f, d, w))
    t = src._replace(name="flags_ragged", nodes=nodes)
    out.append(Case("flags", t, node_queries(t, rng)))
    return out


def family_stop_words():
    out = []
    for seed, scoring, weighting in ((50, 0, 0), (51, 1, 1), (52, 5, 0), (53, 2, 2), (54, 5, 3)):
        src = ragged_tree("stop_words_s%d_w%d" % (scoring, weighting), seed, scoring=scoring, weighting=weighting)
        rng = np.random.RandomState(seed)
        nodes = [(p, f, d, 0.0 if f and rng.uniform() < 0.3 else w) for p, f, d, w in src.nodes]
        t = src._replace(nodes=nodes)
        out.append(Case("stop_words", t, node_queries(t, rng)))
    return out


def family_two_nodes():
    out = []
    for L in (1, 3):
        b = Builder("two_nodes_L%d" % L, 2, L, seed=60 + L)
        b.add(0, weight=3.0)
        out.append(Case("two_nodes", b.tree(), rand_desc(b.rng, 5)))
    return out


FEATURE_COUNTS = (1, 63, 64, 65, 127, 129)


def family_counts():
    t = ragged_tree("counts", 70)
    rng = np.random.RandomState(70)
    pool = node_queries(t, rng, 60, 60)
    return [Case("counts", t._replace(name="counts_n%d" % n), pool[rng.choice(len(pool), n, replace=n > len(pool))]) for n in FEATURE_COUNTS]


def random_tree(seed, k=10, L=6, nodes=1500, stop_words=True, irregular_flags=True):
    """An irregular tree up to ORBvoc's k and L in the reference's recursion order, bounded so that the Python reference descends a
    few hundred queries at every levelsup in about a second."""
    b = Builder("random%d_k%d_L%d" % (seed, k, L), k, L, seed=seed)
    grow(b, 0, 0, lambda rng, depth: rng.randint(2 if depth == 0 else 1, k + 1), 0.3, [nodes])
    t = b.tree()
    rng = np.random.RandomState(seed + 1000)
    out = []
    for p, f, d, w in t.nodes:
        if stop_words and f and rng.uniform() < 0.05:
            w = 0.0
        if irregular_flags and rng.uniform() < 0.01:
            f, w = 1 - f, (w if w else 1.5)
        out.append((p, f, d, w))
    return t._replace(nodes=out)


def family_random():
    out = []
    for seed, k, L in ((1, 10, 6), (2, 10, 6), (3, 7, 5), (4, 20, 3), (5, 2, 10)):
        t = random_tree(seed, k, L)
        out.append(Case("random", t, node_queries(t, np.random.RandomState(seed), 60, 120)[::4]))
    return out


FAMILIES = collections.OrderedDict([
    ("ragged", family_ragged), ("depths", family_depths), ("orders", family_orders), ("ties", family_ties),
    ("last_bits", family_last_bits), ("flags", family_flags), ("stop_words", family_stop_words), ("two_nodes", family_two_nodes),
    ("counts", family_counts), ("random", family_random)])


def levelsups(tree):
    return range(-1, tree.L + 3)


_CACHE = {}


def all_cases():
    if "all" not in _CACHE:
        _CACHE["all"] = [c for fam in FAMILIES.values() for c in fam()]
    return _CACHE["all"]


# ---- corrupt blobs ------------------------------------------------------------------------------------------------------------

def blob_offsets(n):
    pad = lambda v: (v + 63) // 64 * 64
    off, out = 64, {}
    for name, size in (("desc", n * 32), ("weight", n * 8), ("parent", n * 4), ("child0", n * 4), ("nchild", n * 4), ("word", n * 4),
                       ("children", (n - 1) * 4)):
        out[name] = off
        off = pad(off + size)
    out["end"] = off
    return out


def corruptions(blob):
    """[(name, blob)]: single-field corruptions of a valid blob of an irregular tree, each of which a loader must refuse."""
    blob = np.asarray(blob, np.uint8)
    n = int(blob[:64].view(np.int32)[4])
    o = blob_offsets(n)
    i32 = lambda name, cnt: blob[o[name]:o[name] + 4 * cnt].view(np.int32)
    parent, child0, nchild, children = i32("parent", n), i32("child0", n), i32("nchild", n), i32("children", n - 1)
    inner = [i for i in range(1, n) if nchild[i] > 0]
    deep = next(i for i in inner if parent[i] != 0)            # an inner node whose parent is not the root
    last_inner = inner[-1]
    other = next(i for i in inner if i != parent[n - 1])

    def put(name, index, value):
        bad = blob.copy()
        bad[o[name] + 4 * index:o[name] + 4 * index + 4] = np.frombuffer(np.int32(value).tobytes(), np.uint8)
        return bad
    return [
        ("child range past children[]", put("child0", last_inner, n - 1)),
        ("child count past children[]", put("nchild", inner[0], n)),
        ("negative child range", put("child0", inner[0], -4)),
        ("child id 0", put("children", int(child0[deep]), 0)),
        ("child id n", put("children", n - 2, n)),
        ("negative parent", put("parent", n - 1, -2)),
        ("parent n", put("parent", 1, n)),
        ("child list disagrees with parent[]", put("parent", n - 1, other)),
        ("two-node cycle", put("children", int(child0[deep]), int(parent[deep]))),
        ("childless root", put("nchild", 0, 0)),
        ("truncated", blob[:o["end"] - 64].copy()),
        ("truncated inside desc[]", blob[:o["desc"] + 64].copy()),
    ]


# ---- node ids of frames, for the FeatureVector builders ---------------------------------------------------------------------

FV_N = (0, 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 8191, 8192)


def _frame(cap, n_given, ids, rng):
    """One row of `cap` slots: ids in front, every slot past min(n, cap) poisoned with values that differ from slot to slot."""
    n = min(n_given, cap)
    row = (np.uint32(POISON) ^ rng.randint(0, 1 << 16, cap).astype(np.uint32)) | np.uint32(0x80000000)
    ids = np.asarray(ids, np.uint64).astype(np.uint32)
    assert len(ids) == n
    row[:n] = ids
    return row


def _ids(rng, n, kind, mx):
    """n node ids of one pattern whose largest value is exactly mx (when n allows)."""
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "equal":
        return np.full(n, mx, np.uint32)
    if kind == "descending":
        return (np.uint64(mx) - np.arange(n, dtype=np.uint64)).astype(np.uint32) if mx >= n else np.arange(n, dtype=np.uint32)[::-1].copy()
    if kind == "alternating":
        a = np.zeros(n, np.uint32)
        a[::2] = mx
        return a
    a = (rng.randint(0, 1 << 32, n, dtype=np.uint64) % np.uint64(mx + 1)).astype(np.uint32)
    if n:
        a[rng.randint(n)] = mx
    return a


def fv_batch(name, cap, frames, seed):
    """frames: (n as given in d_n, kind, mx)."""
    rng = np.random.RandomState(seed)
    rows = [_frame(cap, n, _ids(rng, min(n, cap), kind, mx), rng) for n, kind, mx in frames]
    return FvBatch(name, cap, np.array([f[0] for f in frames], np.int32), np.array(rows, np.uint32).reshape(len(frames), cap))


ORBVOC_L4, ORBVOC_WORDS = 2047, 1111110                      # 11 bits: node ids at levelsup 4; 21 bits: at word level


def fv_batches_sorted():
    """cap <= 8192: the sorting builder."""
    out = []
    # every n at a cap that holds the largest, ORBvoc-range ids; empty frames between full ones; d_n above cap
    frames = []
    for i, n in enumerate(FV_N):
        frames.append((n, "random", ORBVOC_L4 if i % 2 else ORBVOC_WORDS))
        if n in (8, 512, 8191):
            frames.append((0, "random", 1))
    frames += [(9000, "random", ORBVOC_L4), (0, "zero", 0), (8192, "equal", 0xFFFFFFFF), (8192, "zero", 0), (8192, "descending", 0xFFFFFFFF),
               (8192, "alternating", ORBVOC_WORDS), (8191, "descending", 8190), (1 << 30, "random", 0xFFFFFFFF)]
    out.append(fv_batch("cap8192", 8192, frames, 1))
    # each n with cap = n (and n - 1, 0, n + 5 in the same batch)
    for cap in FV_N[1:-1]:
        frames = [(cap, "random", ORBVOC_WORDS), (0, "zero", 0), (cap - 1, "random", ORBVOC_L4), (cap + 5, "descending", 0xFFFFFFFF),
                  (cap, "zero", 0), (cap, "equal", 77), (cap, "alternating", 0x80000000), (cap, "descending", cap + 3)]
        out.append(fv_batch("cap%d" % cap, cap, frames, 100 + cap))
    # the largest id decides the number of passes: maxima 1, 2^b - 1 and 2^b for every b
    frames = [(65, "random", 1), (65, "alternating", 1)]
    for b in range(1, 33):
        frames.append((65, "random", (1 << b) - 1))
        if b < 32:
            frames.append((64 if b % 2 else 65, "random", 1 << b))
    frames += [(65, "equal", 0xFFFFFFFF), (65, "alternating", 0xFFFFFFFF), (65, "descending", 0xFFFFFFFF), (65, "equal", 0x80000000)]
    out.append(fv_batch("maxima_cap65", 65, frames, 2))
    frames = []
    for b in (1, 2, 11, 12, 21, 22, 31, 32):
        frames += [(513, "random", (1 << b) - 1), (511, "descending", (1 << b) - 1), (600, "alternating", (1 << b) - 1)]
    out.append(fv_batch("maxima_cap513", 513, frames, 3))
    return out


def fv_batches_counting():
    """cap > 8192: the counting builder."""
    out = []
    for cap in (8193, 16000):
        frames = [(cap, "random", ORBVOC_WORDS), (0, "zero", 0), (cap, "random", ORBVOC_L4), (cap + 4000, "random", 0xFFFFFFFF), (8192, "equal", 5),
                  (cap, "zero", 0), (cap, "alternating", 0xFFFFFFFF), (cap, "descending", 0xFFFFFFFF), (1, "equal", 0x80000000), (0, "zero", 0),
                  (cap - 1, "descending", cap + 7)]
        out.append(fv_batch("cap%d" % cap, cap, frames, 200 + cap))
    return out
