"""Plain pointer-tree restatement of the reference's vocabulary path, written from the upstream text and from nothing else:

  Node                      thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:297-329
  loadFromTextFile          TemplatedVocabulary.h:1337-1420
  transform (one feature)   TemplatedVocabulary.h:1217-1259
  transform (a frame)       TemplatedVocabulary.h:1126-1194, ScoringObject.h:74-89 for mustNormalize
  FORB::distance            FORB.cpp:81-101
  BowVector                 BowVector.cpp:34-84
  FeatureVector             FeatureVector.cpp:31-45

Nodes are objects with a list of children, std::map is a dict read out in key order, double is the Python float.  `rules` (a
Rules) switches one reading at a time: REFERENCE is upstream's, every entry of MUTANTS is a wrong one that the cases of
tests/vocab_cases.py must tell apart.  `hits` (a collections.Counter, optional) counts the edges a call reached.

Two places where this file states the PRODUCT's contract because upstream has no defined behaviour:
  * `*nid` is written only when the descent passes level L - levelsup (:1251) or when that level is <= 0 (:1227).  A leaf reached
    above that level leaves the caller's variable as it was, uninitialised in transform(features, ...) (:1151, :1179).  The
    contract (include/pgorb.h: "0 = root") is node 0.  That is the contract, not upstream behaviour.
  * a line without numbers (the trailing newline of a file) makes upstream append a bogus node (:1379-1392); the product skips
    empty lines and so does this loader.
"""
import dataclasses
import math

import numpy as np


@dataclasses.dataclass(frozen=True)
class Rules:
    tie: str = "first"             # sibling tie: the first minimum wins, `d < best_d` (:1244); "last" is `<=`
    nid_shift: int = 0             # nid_level = L - levelsup (:1226); +1 / -1 are the off-by-one readings
    stop: str = "children"         # the descent ends at children.empty() (:328, :1254); "flag" ends it at the isLeaf column
    word_ids: str = "flag"         # word ids count the flagged lines in file order (:1407-1412); "structure": the childless nodes
    unflagged_word: int = 0        # Node() leaves word_id 0 (:316) on a node that was never flagged
    stop_words: str = "drop"       # `w > 0` (:1157, :1185); "keep" is `w >= 0`
    distance_bits: int = 256       # FORB::distance runs over 8 x 32 bits (:92)
    feature_order: str = "append"  # addFeature push_backs in feature order (FeatureVector.cpp:37, :43); "reverse"
    node_order: str = "unsigned"   # NodeId is unsigned int, std::map orders by it; "signed" orders as int32


REFERENCE = Rules()
MUTANTS = {
    "tie=last": Rules(tie="last"),
    "nid_level+1": Rules(nid_shift=1),
    "nid_level-1": Rules(nid_shift=-1),
    "stop=flag": Rules(stop="flag"),
    "word_ids=structure": Rules(word_ids="structure"),
    "unflagged_word=-1": Rules(unflagged_word=-1),
    "stop_words=keep": Rules(stop_words="keep"),
    "distance_bits=248": Rules(distance_bits=248),
    "feature_order=reverse": Rules(feature_order="reverse"),
    "node_order=signed": Rules(node_order="signed"),
}

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)


def _hit(hits, key, n=1):
    if hits is not None:
        hits[key] += n


class Node:
    """:297-329.  `flag` is the isLeaf column as read; upstream does not keep it (only the stop=flag mutant looks at it)."""

    def __init__(self, nid=0):
        self.id = nid
        self.weight = 0.0
        self.children = []
        self.parent = 0
        self.descriptor = 0            # the 32 bytes as one little-endian integer
        self.word_id = 0
        self.flag = False

    def is_leaf(self):
        return not self.children


def descriptor_int(d):
    return int.from_bytes(bytes(bytearray(int(b) & 0xFF for b in d)), "little")


def distance(a, b, rules=REFERENCE):
    """FORB.cpp:81-101: the number of differing bits of the 8 32-bit words."""
    x = a ^ b
    if rules.distance_bits != 256:
        x &= (1 << rules.distance_bits) - 1
    return bin(x).count("1")


class Vocabulary:
    def __init__(self):
        self.k = self.L = 0
        self.scoring = self.weighting = 0
        self.nodes = []
        self.words = []

    # ---- :1337-1420 -------------------------------------------------------------------------------------------------------------
    @classmethod
    def load_text(cls, path, rules=REFERENCE, hits=None):
        v = cls()
        with open(path) as f:
            lines = f.read().split("\n")
        head = lines[0].split()
        v.k, v.L, n1, n2 = int(head[0]), int(head[1]), int(head[2]), int(head[3])
        if v.k < 0 or v.k > 20 or v.L < 1 or v.L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:
            raise ValueError("not a correct text file")
        v.scoring, v.weighting = n1, n2
        v.nodes = [Node(0)]
        depth = [0]
        for line in lines[1:]:
            tok = line.split()
            if not tok:
                continue                                       # (the product's deviation, see the module text)
            nid = len(v.nodes)
            node = Node(nid)
            v.nodes.append(node)
            pid = int(tok[0])
            node.parent = pid
            v.nodes[pid].children.append(nid)
            depth.append(depth[pid] + 1)
            if depth[nid] < depth[nid - 1]:
                _hit(hits, "file_order_not_breadth_first")
            is_leaf = int(tok[1])
            node.descriptor = descriptor_int(int(t) for t in tok[2:34])
            node.weight = float(tok[34]) if len(tok) > 34 else 0.0
            node.flag = is_leaf > 0
            if is_leaf > 0:
                node.word_id = len(v.words)
                v.words.append(node)
        for node in v.nodes[1:]:
            if node.flag and node.children:
                _hit(hits, "flagged_with_children")
            if not node.flag and not node.children:
                _hit(hits, "unflagged_childless")
                node.word_id = rules.unflagged_word
        if len(v.nodes) == 2:
            _hit(hits, "two_node_tree")
        if rules.word_ids == "structure":
            v.words = [n for n in v.nodes[1:] if not n.children]
            for n in v.nodes:
                n.word_id = 0
            for i, n in enumerate(v.words):
                n.word_id = i
        return v

    # ---- :1217-1259 -------------------------------------------------------------------------------------------------------------
    def transform_one(self, feature, levelsup, rules=REFERENCE, hits=None):
        """(word_id, weight, nid) of one descriptor (an integer from descriptor_int); word_id and nid as unsigned 32-bit values."""
        nid_level = self.L - levelsup + rules.nid_shift
        nid = None
        if nid_level <= 0:
            nid = 0
            _hit(hits, "nid_root")
        final_id = 0
        current_level = 0
        while True:
            current_level += 1
            nodes = self.nodes[final_id].children
            if len(nodes) == 1:
                _hit(hits, "single_child")
            elif len(nodes) < self.k:
                _hit(hits, "ragged_arity")
            final_id = nodes[0]
            best_d = distance(feature, self.nodes[final_id].descriptor, rules)
            seen = [best_d]
            for cid in nodes[1:]:
                d = distance(feature, self.nodes[cid].descriptor, rules)
                seen.append(d)
                if d < best_d or (rules.tie == "last" and d == best_d):
                    best_d = d
                    final_id = cid
            if hits is not None:
                for cid in nodes:
                    x = feature ^ self.nodes[cid].descriptor
                    if x and not x & ((1 << 248) - 1):
                        _hit(hits, "sibling_differs_in_the_last_bit_only" if x == 1 << 255 else "sibling_differs_in_the_last_byte_only")
            if seen.count(best_d) > 1:
                _hit(hits, "tie_level_%d" % current_level)
                if best_d == 0:
                    _hit(hits, "tie_at_distance_0")
            if current_level == nid_level:
                nid = final_id
                _hit(hits, "nid_at_the_leaf" if self.nodes[final_id].is_leaf() else "nid_above_the_leaf")
            node = self.nodes[final_id]
            if rules.stop == "flag":
                if node.flag or node.is_leaf():
                    break
            elif node.is_leaf():
                break
        if current_level < self.L:
            _hit(hits, "leaf_at_depth_%d_of_%d" % (current_level, self.L))
        if current_level == self.L:
            _hit(hits, "leaf_at_depth_L")
        if nid is None:
            nid = 0                                            # the contract, not upstream (see the module text)
            _hit(hits, "nid_never_reached")
        if not node.flag and node.is_leaf():
            _hit(hits, "descent_ends_unflagged")
        if node.weight == 0:
            _hit(hits, "stop_word")
        return node.word_id & 0xFFFFFFFF, node.weight, nid & 0xFFFFFFFF

    def transform_features(self, features, levelsup, rules=REFERENCE, hits=None):
        """transform_one of every row of `features` ([n, 32] bytes) as arrays (word u32, weight f64, node u32)."""
        n = len(features)
        _hit(hits, "features_%d" % n)
        word, weight, node = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.uint32)
        for i in range(n):
            word[i], weight[i], node[i] = self.transform_one(descriptor_int(features[i]), levelsup, rules, hits)
        return word, weight, node

    # ---- :1126-1194 -------------------------------------------------------------------------------------------------------------
    def transform(self, features, levelsup, rules=REFERENCE, hits=None):
        """(BowVector, FeatureVector) of a frame as ordered lists: [(word id, value)], [(node id, [feature, ...])]."""
        triples = [self.transform_one(descriptor_int(f), levelsup, rules, hits) for f in features]
        return accumulate(triples, self.scoring, self.weighting, rules)


def accumulate(triples, scoring, weighting, rules=REFERENCE):
    """The loop of :1145-1193 over the per-feature (word id, weight, node id)."""
    v, fv = {}, {}
    tf = weighting in (TF, TF_IDF)
    for i_feature, (wid, w, nid) in enumerate(triples):
        if w > 0 or (rules.stop_words == "keep" and w >= 0):
            if tf:
                v[wid] = v[wid] + w if wid in v else w         # addWeight, BowVector.cpp:34-46
            elif wid not in v:
                v[wid] = w                                     # addIfNotExist, :50-58
            add_feature(fv, nid, i_feature, rules)
    must = scoring != DOT_PRODUCT                              # ScoringObject.h:74-89
    keys = sorted(v)
    if tf and v and not must:                                  # :1164-1170
        nd = float(len(v))
        for k in keys:
            v[k] /= nd
    if must:                                                   # BowVector::normalize, :62-84
        norm = 0.0
        if scoring != L2_NORM:
            for k in keys:
                norm += math.fabs(v[k])
        else:
            for k in keys:
                norm += v[k] * v[k]
            norm = math.sqrt(norm)
        if norm > 0.0:
            for k in keys:
                v[k] /= norm
    return [(k, v[k]) for k in keys], ordered(fv, rules)


def add_feature(fv, nid, i_feature, rules=REFERENCE):
    """FeatureVector.cpp:31-45."""
    if nid not in fv:
        fv[nid] = []
    if rules.feature_order == "reverse":
        fv[nid].insert(0, i_feature)
    else:
        fv[nid].append(i_feature)


def ordered(fv, rules=REFERENCE):
    """The map read from begin() to end(): NodeId is unsigned int."""
    if rules.node_order == "signed":
        keys = sorted(fv, key=lambda k: k - (1 << 32) if k >= (1 << 31) else k)
    else:
        keys = sorted(fv)
    return [(k, list(fv[k])) for k in keys]


def feature_vector(node_ids, rules=REFERENCE):
    """The FeatureVector of a frame whose feature i lies in node node_ids[i] (every feature kept)."""
    fv = {}
    for i, nid in enumerate(node_ids):
        add_feature(fv, int(nid) & 0xFFFFFFFF, i, rules)
    return ordered(fv, rules)


def bow_arrays(bow):
    return np.array([k for k, _ in bow], np.uint32), np.array([x for _, x in bow], np.float64)


def csr(fv):
    """A FeatureVector as (node u32 [nfv], start i32 [nfv + 1], feat u32 [sum])."""
    node = np.array([k for k, _ in fv], np.uint32)
    start = np.zeros(len(fv) + 1, np.int32)
    feat = []
    for g, (_, fs) in enumerate(fv):
        feat.extend(fs)
        start[g + 1] = len(feat)
    return node, start, np.array(feat, np.uint32)
