"""The vocabulary path (pilotguru_amd/csrc/bow.hip: the text loader, pack_blob, view_blob, k_vocab_validate, k_bow_transform;
node_match.hip: k_feature_vectors, k_feature_vectors_sorted) against the plain pointer-tree reference (tests/vocab_reference.py) on
irregular trees and constructed node-id frames (tests/vocab_cases.py).  Every comparison is exact: integers as integers, doubles
as bit patterns."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocab_cases as VC  # noqa: E402
import vocab_reference as VR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pilotguru_amd import vocab as V  # noqa: E402

EDGES = {
    "ragged": ["single_child", "ragged_arity", "file_order_not_breadth_first", "leaf_at_depth_L", "leaf_at_depth_2_of_4"],
    "depths": ["leaf_at_depth_%d_of_6" % d for d in range(1, 6)] + ["leaf_at_depth_L", "nid_root", "nid_above_the_leaf", "nid_at_the_leaf",
                                                                      "nid_never_reached"],
    "orders": ["file_order_not_breadth_first"],
    "ties": ["tie_level_1", "tie_level_2", "tie_level_3", "tie_at_distance_0"],
    "last_bits": ["sibling_differs_in_the_last_byte_only", "sibling_differs_in_the_last_bit_only"],
    "flags": ["flagged_with_children", "unflagged_childless", "descent_ends_unflagged"],
    "stop_words": ["stop_word"],
    "two_nodes": ["two_node_tree", "single_child", "nid_never_reached", "nid_at_the_leaf", "nid_root"],
    "counts": ["features_%d" % n for n in VC.FEATURE_COUNTS],
    "random": ["single_child", "ragged_arity", "leaf_at_depth_L", "leaf_at_depth_1_of_6", "leaf_at_depth_5_of_6", "stop_word",
               "descent_ends_unflagged", "flagged_with_children", "nid_never_reached"],
}


def _text(case, tmp_path):
    return VC.write_text(case.tree, os.path.join(str(tmp_path), case.tree.name + ".txt"))


def run_reference(case, path, rules=VR.REFERENCE, hits=None):
    """Per levelsup: word, weight, node of every query, and the frame's BowVector and FeatureVector, all as arrays."""
    voc = VR.Vocabulary.load_text(path, rules, hits)
    out = []
    for lu in VC.levelsups(case.tree):
        word, weight, node = voc.transform_features(case.queries, lu, rules, hits)
        bow, fv = VR.accumulate(list(zip(word.tolist(), weight.tolist(), node.tolist())), voc.scoring, voc.weighting, rules)
        out.append((word, weight, node) + VR.bow_arrays(bow) + VR.csr(fv))
    return out


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                                    for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """[(case, text file, reference results)] of every constructed and random tree."""
    d = tmp_path_factory.mktemp("vocab_edges")
    out = []
    for c in VC.all_cases():
        path = _text(c, d)
        out.append((c, path, run_reference(c, path)))
    return out


# ---- the cases and the reference themselves -------------------------------------------------------------------------------------

def test_every_family_reaches_its_edges(tmp_path):
    missing = {}
    for fam, make in VC.FAMILIES.items():
        hits = collections.Counter()
        for c in make():
            run_reference(c, _text(c, tmp_path), hits=hits)
        lost = [e for e in EDGES[fam] if not hits[e]]
        if lost:
            missing[fam] = (lost, dict(hits))
    assert not missing, missing


def test_every_rule_mutant_is_caught(refs):
    small = [(c, p, w) for c, p, w in refs if c.family not in ("random", "counts")]
    frames = [b for b in VC.fv_batches_sorted() if b.name == "maxima_cap65"][0]
    want_fv = [VR.feature_vector(row[:min(n, frames.cap)]) for n, row in zip(frames.n, frames.node)]
    survivors = []
    for name, rules in VR.MUTANTS.items():
        caught = [c.tree.name for c, p, w in small if not same(w, run_reference(c, p, rules))]
        caught += ["fv"] * (want_fv != [VR.feature_vector(row[:min(n, frames.cap)], rules) for n, row in zip(frames.n, frames.node)])
        if not caught:
            survivors.append(name)
    assert not survivors, survivors


def test_node_id_frames_cover_the_listed_shapes():
    batches = VC.fv_batches_sorted() + VC.fv_batches_counting()
    used = set(min(int(n), b.cap) for b in batches for n in b.n)
    assert set(VC.FV_N) <= used and set(b.cap for b in batches) >= set(VC.FV_N[1:]) | {8193, 16000}
    assert any(int(n) > b.cap for b in batches for n in b.n)
    bits = set()
    for b in batches:
        for n, row in zip(b.n, b.node):
            ids = row[:min(int(n), b.cap)]
            if len(ids):
                bits.add((int(ids.max()).bit_length(), int(ids.max()) & (int(ids.max()) + 1) == 0))
            assert (row[min(int(n), b.cap):] >= 0x80000000).all()                # poison past n
    assert set((w, True) for w in range(1, 33)) <= bits and set((w + 1, False) for w in range(1, 32)) <= bits


def test_reference_equals_the_oracle(refs, oracle):
    for c, path, want in refs:
        ora = oracle.VocabOracle(path)
        voc = VR.Vocabulary.load_text(path)
        assert (ora.k, ora.L, ora.nnodes, ora.nwords) == (voc.k, voc.L, len(voc.nodes), len(voc.words)), c.tree.name
        for lu, w in zip(VC.levelsups(c.tree), want):
            word, weight, node = ora.transform_features(c.queries, lu)
            assert np.array_equal(word, w[0]) and weight.tobytes() == w[1].tobytes() and np.array_equal(node, w[2]), (c.tree.name, lu)
            (bid, bval), fv = ora.transform(c.queries, lu)
            assert np.array_equal(bid, w[3]) and bval.tobytes() == w[4].tobytes(), (c.tree.name, lu)
            assert all(g.dtype == r.dtype and np.array_equal(g, r) for g, r in zip(fv, w[5:])), (c.tree.name, lu)


# ---- the product's host side --------------------------------------------------------------------------------------------------

def blob_word(node):
    """What the blob's word[] holds for a reference node: the word a descent ending there returns; a flagged node's id even when it
    has children (it used one up); -1 for an unflagged inner node, which no descent returns."""
    return node.word_id if node.flag or node.is_leaf() else -1


def test_unflagged_childless_node_is_word_0(tmp_path):
    """TemplatedVocabulary.h:316 and :1407-1415: a childless line without the leaf flag keeps Node()'s word_id 0, and a descent that
    ends there returns word 0; a flagged line that later receives children still uses up a word id."""
    c = [c for c in VC.family_flags() if c.tree.name == "flags_small"][0]
    voc = V.ORBVocabulary(text_file=_text(c, tmp_path))
    u = V.unpack_vocabulary(voc.blob())
    assert u["nchild"].tolist() == [4, 0, 2, 0, 0, 0, 1, 0]
    assert u["word"].tolist() == [-1, 0, 0, 1, 0, 2, -1, 0] and voc.nwords == 3
    ref = VR.Vocabulary.load_text(_text(c, tmp_path))
    assert [blob_word(n) for n in ref.nodes[1:]] == u["word"].tolist()[1:]
    desc, weight, parent, flag = VC.arrays(c.tree)
    assert np.array_equal(V.pack_vocabulary(4, 3, desc, weight, parent, leaf_flag=flag), voc.blob())


def test_loader_equals_the_reference_tree(refs):
    for c, path, _ in refs:
        ref = VR.Vocabulary.load_text(path)
        voc = V.ORBVocabulary(text_file=path)
        blob = voc.blob()
        u = V.unpack_vocabulary(blob)
        n = len(ref.nodes)
        assert (voc.k, voc.L, voc.nnodes, voc.nwords, voc.scoring, voc.weighting) == (ref.k, ref.L, n, len(ref.words), ref.scoring, ref.weighting)
        assert (u["k"], u["L"], u["nnodes"], u["nwords"]) == (ref.k, ref.L, n, len(ref.words)), c.tree.name
        seen = 0
        for i, node in enumerate(ref.nodes):
            ch = u["children"][u["child0"][i]:u["child0"][i] + u["nchild"][i]].tolist()
            assert ch == node.children, (c.tree.name, i)
            seen += len(ch)
            if i:
                assert u["parent"][i] == node.parent and VR.descriptor_int(u["desc"][i]) == node.descriptor, (c.tree.name, i)
                assert u["weight"][i:i + 1].tobytes() == np.float64(node.weight).tobytes(), (c.tree.name, i)
                assert u["word"][i] == blob_word(node), (c.tree.name, i, u["word"][i], blob_word(node))
        assert seen == n - 1 and u["parent"][0] == -1 and u["word"][0] == -1
        # the blob through the C ABI and back
        assert np.array_equal(V.ORBVocabulary(blob=blob).blob(), blob), c.tree.name
        # the Python packer: with the file's flags always; without them where the flags are the structure
        desc, weight, parent, flag = VC.arrays(c.tree)
        t = c.tree
        assert np.array_equal(V.pack_vocabulary(t.k, t.L, desc, weight, parent, t.scoring, t.weighting, leaf_flag=flag), blob), t.name
        if np.array_equal(flag[1:] != 0, np.bincount(parent[1:], minlength=n)[1:] == 0):
            assert np.array_equal(V.pack_vocabulary(t.k, t.L, desc, weight, parent, t.scoring, t.weighting), blob), t.name


def test_trailing_newline_and_empty_lines_are_skipped(tmp_path):
    c = VC.family_flags()[0]
    a = V.ORBVocabulary(text_file=_text(c, tmp_path)).blob()
    path = VC.write_text(c.tree, os.path.join(str(tmp_path), "nl.txt"), trailing_newline=True)
    assert np.array_equal(V.ORBVocabulary(text_file=path).blob(), a)
    assert len(VR.Vocabulary.load_text(path).nodes) == len(c.tree.nodes) + 1


def test_host_accumulation_equals_the_reference(refs):
    for c, path, want in refs:
        for lu, w in zip(VC.levelsups(c.tree), want):
            (bid, bval), fv = V.bow_vectors(w[0], w[1], w[2], c.tree.scoring, c.tree.weighting)
            assert bid.dtype == w[3].dtype and np.array_equal(bid, w[3]) and bval.tobytes() == w[4].tobytes(), (c.tree.name, lu)
            assert all(g.dtype == r.dtype and np.array_equal(g, r) for g, r in zip(fv, w[5:])), (c.tree.name, lu)
    # node ids a tree cannot give: the FeatureVector's order is that of unsigned ids
    b = [b for b in VC.fv_batches_sorted() if b.name == "maxima_cap65"][0]
    for n, row in zip(b.n, b.node):
        ids = row[:min(int(n), b.cap)]
        _, fv = V.bow_vectors(np.arange(len(ids), dtype=np.uint32), np.ones(len(ids)), ids, 0, 0)
        assert all(np.array_equal(g, r) for g, r in zip(fv, VR.csr(VR.feature_vector(ids))))


def _irregular_blob(tmp_path):
    c = [c for c in VC.family_flags() if c.tree.name == "flags_ragged"][0]
    return V.ORBVocabulary(text_file=_text(c, tmp_path)).blob()


def test_view_blob_refuses_single_field_corruptions(tmp_path):
    blob = _irregular_blob(tmp_path)
    V.ORBVocabulary(blob=blob)
    accepted = []
    for name, bad in VC.corruptions(blob):
        try:
            V.ORBVocabulary(blob=bad)
            accepted.append(name)
        except ValueError:
            pass
    assert not accepted, accepted


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------

SENTINEL_U32, SENTINEL_F64 = 0xA5A5A5A5, -7.25


@pytest.fixture(scope="module")
def ext():
    import pilotguru_amd as pg
    e = pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=2)
    yield e
    e.close()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tp(t):
    return C.c_void_p(t.data_ptr())


def gpu_transform(ext, queries, levelsup, device):
    """word, weight, node of pgorb_bow_transform (host arrays) or pgorb_bow_transform_device, with 7 sentinel slots past n that
    must come back untouched."""
    import torch
    n, pad = len(queries), 7
    q = np.ascontiguousarray(queries, np.uint8)
    if device:
        d = torch.from_numpy(q).cuda()
        word = torch.full((n + pad,), SENTINEL_U32 - (1 << 32), dtype=torch.int32, device="cuda")
        node = word.clone()
        weight = torch.full((n + pad,), SENTINEL_F64, dtype=torch.float64, device="cuda")
        ext._check(ext._L.pgorb_bow_transform_device(ext._h, _tp(d), n, levelsup, _tp(word), _tp(weight), _tp(node), _stream()))
        torch.cuda.synchronize()
        word, weight, node = word.cpu().numpy().view(np.uint32), weight.cpu().numpy(), node.cpu().numpy().view(np.uint32)
    else:
        word, node = np.full(n + pad, SENTINEL_U32, np.uint32), np.full(n + pad, SENTINEL_U32, np.uint32)
        weight = np.full(n + pad, SENTINEL_F64, np.float64)
        p = lambda a: C.c_void_p(a.ctypes.data)
        ext._check(ext._L.pgorb_bow_transform(ext._h, p(q), n, levelsup, p(word), p(weight), p(node)))
    assert (word[n:] == SENTINEL_U32).all() and (node[n:] == SENTINEL_U32).all() and (weight[n:] == SENTINEL_F64).all()
    return word[:n], weight[:n], node[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(VC.FAMILIES))
def test_gpu_descent_equals_the_reference(ext, tmp_path, family):
    """k_bow_transform through pgorb_bow_transform and pgorb_bow_transform_device: word, weight bits and node of every query at
    every levelsup from -1 to L + 2."""
    for c in VC.FAMILIES[family]():
        path = _text(c, tmp_path)
        want = run_reference(c, path)
        voc = V.ORBVocabulary(text_file=path)
        voc.upload(ext)
        for lu, w in zip(VC.levelsups(c.tree), want):
            for device in (False, True):
                word, weight, node = gpu_transform(ext, c.queries, lu, device)
                bad = np.nonzero((word != w[0]) | (weight.view(np.uint64) != w[1].view(np.uint64)) | (node != w[2]))[0]
                assert not len(bad), (c.tree.name, lu, device, bad[:5], word[bad[:5]], w[0][bad[:5]], node[bad[:5]], w[2][bad[:5]])
        (bid, bval), fv = voc.transform(c.queries, 1)
        w = want[list(VC.levelsups(c.tree)).index(1)]
        assert np.array_equal(bid, w[3]) and bval.tobytes() == w[4].tobytes() and all(np.array_equal(g, r) for g, r in zip(fv, w[5:]))


@pytest.mark.gpu
def test_gpu_upload_refuses_every_corruption(tmp_path):
    """pgorb_vocab_upload_device (k_vocab_validate) on each blob that view_blob refused: PGORB_E_ARG and no vocabulary resident.
    The transform is called only to see it return an error; no descent ever runs on a refused blob."""
    import torch
    import pilotguru_amd as pg
    blob = _irregular_blob(tmp_path)
    for name, bad in VC.corruptions(blob):
        with pytest.raises(ValueError):
            V.ORBVocabulary(blob=bad)
        e = pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)
        try:
            t = torch.from_numpy(bad).cuda()
            rc = e._L.pgorb_vocab_upload_device(e._h, _tp(t), t.numel(), _stream())
            assert rc == -1, (name, rc)                                           # PGORB_E_ARG
            d = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
            w = torch.zeros(4, dtype=torch.int32, device="cuda"); wt = torch.zeros(4, dtype=torch.float64, device="cuda")
            nd = torch.zeros(4, dtype=torch.int32, device="cuda")
            assert e._L.pgorb_bow_transform_device(e._h, _tp(d), 4, 1, _tp(w), _tp(wt), _tp(nd), _stream()) != 0, name
        finally:
            e.close()
    # the intact blob by the same way is taken
    e = pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)
    t = torch.from_numpy(blob).cuda()
    assert e._L.pgorb_vocab_upload_device(e._h, _tp(t), t.numel(), _stream()) == 0
    e.close()


GUARD = 0x5EC0DE55                                         # (below 2^31: the same value as int32 and as uint32)


def gpu_feature_vectors(ext, b):
    """pgorb_feature_vectors_batch_device on one batch; the outputs carry one guard row in front and one behind.  Returns the names
    of the frames that differ from the reference's CSR."""
    import torch
    F, cap = len(b.n), b.cap
    g = GUARD
    node = torch.from_numpy(b.node.view(np.int32)).cuda()
    n = torch.from_numpy(b.n).cuda()
    fvn = torch.full((F + 2, cap), g, dtype=torch.int32, device="cuda")
    fvf = torch.full((F + 2, cap), g, dtype=torch.int32, device="cuda")
    fvs = torch.full((F + 2, cap + 1), g, dtype=torch.int32, device="cuda")
    nfv = torch.full((F + 2,), g, dtype=torch.int32, device="cuda")
    ext._check(ext._L.pgorb_feature_vectors_batch_device(ext._h, _tp(node), _tp(n), F, cap, _tp(fvn[1]), _tp(fvs[1]), _tp(fvf[1]), _tp(nfv[1:]), _stream()))
    torch.cuda.synchronize()
    fvn, fvf, fvs, nfv = [t.cpu().numpy() for t in (fvn, fvf, fvs, nfv)]
    bad = []
    for a in (fvn, fvf, fvs):
        if not ((a[0] == g).all() and (a[-1] == g).all()):
            bad.append("guard rows")
    if nfv[0] != g or nfv[-1] != g:
        bad.append("guard counts")
    for f in range(F):
        m = min(int(b.n[f]), cap)
        rn, rs, rf = VR.csr(VR.feature_vector(b.node[f, :m]))
        k = int(nfv[1 + f])
        ok = (k == len(rn) and np.array_equal(fvn[1 + f, :k].view(np.uint32), rn) and np.array_equal(fvs[1 + f, :k + 1], rs) and
              np.array_equal(fvf[1 + f, :m].view(np.uint32), rf))
        if not ok:
            bad.append("frame %d (n %d, nfv %d, reference %d)" % (f, int(b.n[f]), k, len(rn)))
    return bad


@pytest.mark.gpu
def test_gpu_feature_vectors_sorting_form(ext):
    """k_feature_vectors_sorted (cap <= 8192): nfv, fvNode[:nfv], fvStart[:nfv + 1], fvFeat[:n] of every frame."""
    failed = {b.name: bad for b in VC.fv_batches_sorted() for bad in [gpu_feature_vectors(ext, b)] if bad}
    assert not failed, failed


@pytest.mark.gpu
def test_gpu_feature_vectors_counting_form(ext):
    """k_feature_vectors takes over above 8192 features per frame; above 16000 the call is refused."""
    import torch
    failed = {b.name: bad for b in VC.fv_batches_counting() for bad in [gpu_feature_vectors(ext, b)] if bad}
    assert not failed, failed
    t = torch.zeros(16001 + 1, dtype=torch.int32, device="cuda")
    assert ext._L.pgorb_feature_vectors_batch_device(ext._h, _tp(t), _tp(t), 1, 16001, _tp(t), _tp(t), _tp(t), _tp(t), _stream()) == -6   # PGORB_E_LIMIT


def _counting_child():
    import pilotguru_amd as pg
    e = pg.ORBextractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240)
    batches = VC.fv_batches_sorted()
    failed = {b.name: bad for b in batches for bad in [gpu_feature_vectors(e, b)] if bad}
    e.close()
    print("counting form: %d batches, %d differ %r" % (len(batches), len(failed), failed))
    return 1 if failed else 0


@pytest.mark.gpu
def test_gpu_feature_vectors_counting_form_at_small_caps():
    """The counting form on the frames of the sorting form: PGORB_FV_COUNTING is read once per process, so one child process runs
    them all."""
    assert os.environ.get("PGORB_FV_COUNTING") is None
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--counting-child"], env=dict(os.environ, PGORB_FV_COUNTING="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "batches, 0 differ" in out, (r.returncode, out[-2000:])


def _bow_scene():
    """An irregular tree without stop words (so that every feature stays in the FeatureVector) and four frames in the layout of
    pgorb_extract_batch_device whose descriptors are noisy copies of a shared pool near the tree's nodes; one frame is empty."""
    from matcher_cases import keys
    tree = VC.random_tree(9, 10, 6, stop_words=False)._replace(name="e2e")
    tree = tree._replace(nodes=[(p, f, d, w if w > 0 else 2.0) for p, f, d, w in tree.nodes])
    rng = np.random.RandomState(9)
    B, cap = 4, 700
    nh = np.array([650, 700, 0, 431], np.int32)
    descs = np.array([d for _, _, d, _ in tree.nodes], np.uint8)
    base = np.array([VC.near(rng, descs[rng.randint(len(descs))], rng.randint(0, 30)) for _ in range(cap)], np.uint8)
    desc = rng.randint(0, 256, (B, cap, 32)).astype(np.uint8)                   # slots past n stay random
    kps = np.zeros((B, cap), keys([0], [0]).dtype)
    for f in range(B):
        order = rng.permutation(cap)[:nh[f]]
        for j, i in enumerate(order):
            desc[f, j] = VC.near(rng, base[i], rng.randint(0, 25))
        kps[f] = keys(rng.uniform(20, 300, cap), rng.uniform(20, 220, cap), 0, rng.uniform(0, 360, cap) if f != 1 else 40.0)
    return tree, desc, kps, nh


@pytest.mark.gpu
def test_gpu_search_by_bow_over_an_irregular_tree(ext, tmp_path):
    """Descriptors on the device -> pgorb_bow_transform_device -> pgorb_feature_vectors_batch_device ->
    pgorb_search_by_bow_batch_device on an irregular tree == tests/matcher_reference.py's SearchByBoW fed the reference's
    FeatureVectors."""
    import torch
    import matcher_reference as MR
    tree, desc, kps, nh = _bow_scene()
    B, cap, levelsup = len(nh), desc.shape[1], 4
    rng = np.random.RandomState(10)
    path = VC.write_text(tree, os.path.join(str(tmp_path), "e2e.txt"))
    ref = VR.Vocabulary.load_text(path)
    V.ORBVocabulary(text_file=path).upload(ext)
    d_desc, d_kps, d_n = torch.from_numpy(desc).cuda(), torch.from_numpy(kps.view(np.uint8).reshape(B, cap, 28)).cuda(), torch.from_numpy(nh).cuda()
    word = torch.empty((B, cap), dtype=torch.int32, device="cuda"); wt = torch.empty((B, cap), dtype=torch.float64, device="cuda")
    node = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    L, hdl, s = ext._L, ext._h, _stream()
    ext._check(L.pgorb_bow_transform_device(hdl, _tp(d_desc), B * cap, levelsup, _tp(word), _tp(wt), _tp(node), s))
    fvn = torch.empty((B, cap), dtype=torch.int32, device="cuda"); fvs = torch.empty((B, cap + 1), dtype=torch.int32, device="cuda")
    fvf = torch.empty((B, cap), dtype=torch.int32, device="cuda"); nfv = torch.empty(B, dtype=torch.int32, device="cuda")
    ext._check(L.pgorb_feature_vectors_batch_device(hdl, _tp(node), _tp(d_n), B, cap, _tp(fvn), _tp(fvs), _tp(fvf), _tp(nfv), s))
    torch.cuda.synchronize()
    FV = []
    for f in range(B):
        fv = VR.csr(ref.transform(desc[f, :nh[f]], levelsup)[1])
        k = int(nfv[f])
        assert k == len(fv[0]) and np.array_equal(fvn[f, :k].cpu().numpy().view(np.uint32), fv[0]), f
        assert np.array_equal(fvs[f, :k + 1].cpu().numpy(), fv[1]) and np.array_equal(fvf[f, :nh[f]].cpu().numpy().view(np.uint32), fv[2]), f
        FV.append(fv)
    assert len(FV[0][0]) > 5 and max(np.diff(FV[0][1])) > 3
    pairs = np.array([(0, 1), (1, 0), (0, 3), (3, 1), (2, 0), (0, 2), (1, 1)], np.int32)
    npairs = len(pairs)
    valid_np = (rng.uniform(size=(npairs, cap)) > 0.2).astype(np.uint8)
    pkf, pf = torch.from_numpy(pairs[:, 0].copy()).cuda(), torch.from_numpy(pairs[:, 1].copy()).cuda()
    valid = torch.from_numpy(valid_np).cuda()
    mt = torch.empty((npairs, cap), dtype=torch.int32, device="cuda"); nm = torch.empty(npairs, dtype=torch.int32, device="cuda")
    total = 0
    for ratio, ori in ((0.7, True), (0.9, False)):
        ext._check(L.pgorb_search_by_bow_batch_device(hdl, _tp(d_kps), _tp(d_desc), _tp(d_n), cap, _tp(fvn), _tp(fvs), _tp(fvf), _tp(nfv), _tp(pkf), _tp(pf),
                                                      npairs, _tp(valid), ratio, int(ori), _tp(mt), _tp(nm), s))
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(pairs):
            onm, om = MR.search_by_bow(desc[a, :nh[a]], kps[a, :nh[a]]["angle"], valid_np[j, :nh[a]], FV[a], desc[b, :nh[b]], kps[b, :nh[b]]["angle"],
                                       FV[b], np.float32(ratio), ori)
            assert int(nm[j]) == onm and np.array_equal(mt[j, :nh[b]].cpu().numpy(), om), "pair %d (%d, %d) ratio %g" % (j, a, b, ratio)
            total += onm
    assert total > 200


if __name__ == "__main__":
    if sys.argv[1:] == ["--counting-child"]:
        sys.exit(_counting_child())
