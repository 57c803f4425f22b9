"""Worlds and edit lists for the map edits (tests/test_map_edits.py): constructed cases, each the smallest world that separates one
rule; seeded random worlds; a restatement of the kernel's DECOMPOSITION (components, the bag, the last-writer commit, plan then
commit) in plain arrays; and the runners of the device and host forms."""
import ctypes as C
import dataclasses

import numpy as np

import map_edit_reference as R

SENT = -77
KEYS = ("kf_point", "point_bad", "visible", "found", "replaced", "obs_start_out", "obs_frame_out", "obs_idx_out", "ref_obs_out", "edit_status",
        "touched", "select_out", "info")
ORDER5 = [2, 0, 4, 1, 3]                  # address ranks of key frames 0 .. 4: by rank the key frames come 1, 3, 0, 4, 2


@dataclasses.dataclass
class Case:
    name: str
    a: dict
    edits: np.ndarray
    obs_cap_out: int = None               # None = exactly what the reference needs
    select_bits: int = R.TOUCH_CHANGED | R.TOUCH_SURVIVOR
    sel_cap: int = None                   # None = npoints


def E(*rows):
    out = np.zeros(len(rows), R.EDIT_DTYPE)
    for k, r in enumerate(rows):
        out[k] = tuple(r) + (0,) * (4 - len(r))
    return out


def world(nkf, nslots, lists, order=None, bad=(), ref=None, visible=None, found=None, slots=None, replaced=None):
    """lists[p] = [(kf, idx) or (kf, idx, 0 = dead)], put into address-rank order here; a live entry of a point fills its slot unless
    `slots` {(kf, idx): point} says otherwise; ref[p] = the key frame of mpRefKF (default: the first entry)"""
    n = np.full(nkf, nslots, np.int32) if np.isscalar(nslots) else np.array(nslots, np.int32)
    cap = int(n.max())
    rank = np.array(order if order is not None else range(nkf))
    npoints = len(lists)
    kf_point = np.full((nkf, cap), -1, np.int32)
    st, of, oi, lv, ro = [0], [], [], [], []
    for p, lst in enumerate(lists):
        lst = sorted([tuple(x) + (1,) * (3 - len(x)) for x in lst], key=lambda x: (rank[x[0]], x[0]))
        r = -1
        for k, (f, i, live) in enumerate(lst):
            of.append(f); oi.append(i); lv.append(live)
            if live and p not in bad:
                kf_point[f, i] = p
            if ref is not None and p in ref and ref[p] == f:
                r = k
        if (ref is None or p not in ref) and lst:
            r = 0
        ro.append(r)
        st.append(len(of))
    for (f, i), v in (slots or {}).items():
        kf_point[f, i] = v
    i32 = lambda x: np.array(x, np.int32).reshape(-1)
    pb = np.zeros(npoints, np.uint8)
    pb[list(bad)] = 1
    return dict(n=n, order=None if order is None else i32(order), cap=cap, kf_point=kf_point, point_bad=pb,
                visible=i32(visible if visible is not None else [10 + p for p in range(npoints)]),
                found=i32(found if found is not None else [5 + p for p in range(npoints)]),
                replaced=i32(replaced if replaced is not None else [-1] * npoints), obs_start=i32(st), obs_frame=i32(of), obs_idx=i32(oi),
                obs_live=np.array(lv, np.uint8).reshape(-1), ref_obs=i32(ro), nobs=len(of), kf_id=np.arange(nkf, dtype=np.uint64) * 3 + 7,
                first_kf_id=i32([0] * npoints))


def cases():
    out = []
    add = lambda name, a, edits, **kw: out.append(Case(name, a, edits, **kw))
    w = lambda lists, **kw: world(5, 8, lists, ORDER5, **kw)
    add("add_front", w([[(0, 0), (4, 0)], [(2, 1)]]), E((R.ADD, 0, 1, 3)))
    add("add_middle", w([[(1, 0), (2, 0)], [(2, 1)]]), E((R.ADD, 0, 0, 3)))
    add("add_end", w([[(0, 0), (4, 0)], [(3, 1)]]), E((R.ADD, 0, 2, 3)))
    add("add_already_observed", w([[(0, 2), (1, 2)]]), E((R.ADD, 0, 0, 5)))
    add("replace_disjoint", w([[(0, 1), (1, 1)], [(2, 2), (3, 2), (4, 2)]]), E((R.REPLACE, 0, 1)))
    add("replace_shared_key_frame", w([[(0, 1), (1, 1)], [(1, 2), (2, 0)], [(3, 3)]], slots={(1, 2): 2}), E((R.REPLACE, 0, 1)))
    add("self_replace", w([[(0, 1), (1, 1)], [(2, 2)]]), E((R.REPLACE, 0, 0)))
    add("chain", w([[(0, 0)], [(1, 1), (0, 4)], [(2, 2)]]), E((R.REPLACE, 0, 1), (R.REPLACE, 1, 2)))
    add("star_second_brings_a_key_frame_again", w([[(0, 0)], [(0, 3), (1, 1)], [(2, 2)]]), E((R.REPLACE, 0, 2), (R.REPLACE, 1, 2)))
    add("loser_already_bad", w([[], [(2, 2), (3, 2)]], bad=(0,), visible=[5, 10], found=[3, 6]), E((R.REPLACE, 0, 1)))
    add("dangling_slot_collision", w([[(2, 3), (0, 0), (1, 0), (3, 0)], [(2, 3), (0, 1)]], slots={(2, 3): 1}), E((R.ERASE, 0, 2), (R.ADD, 1, 2, 3)))
    add("erase_moves_reference", w([[(1, 0), (3, 0), (0, 0), (4, 0)]], ref={0: 1}), E((R.ERASE, 0, 1)))
    add("erase_three_to_two_then_again", w([[(0, 0), (1, 0), (2, 0)], [(3, 3)]], ref={0: 1}), E((R.ERASE, 0, 0), (R.ERASE, 0, 1)))
    add("bad_point_added_again_keeps_reference", w([[(0, 0), (1, 0), (2, 0)]], ref={0: 1}), E((R.ERASE, 0, 0), (R.ADD, 0, 1, 6)))
    add("set_bad_clears_a_foreign_slot", w([[(0, 0), (1, 1), (2, 2)], [(3, 3), (4, 3), (0, 5)]], slots={(2, 2): 1}), E((R.ERASE, 0, 0)))
    add("erase_last_observation", w([[(0, 0)], [(1, 1)]]), E((R.ERASE, 0, 0)))
    add("erase_unlisted_key_frame", w([[(0, 0), (1, 0), (2, 0), (4, 0)]]), E((R.ERASE, 0, 3)))
    # one slot's Fuse chain: the query is ADDED, the next MERGED into it, the third REPLACES it
    add("fuse_chain_on_one_slot", w([[(0, 0), (1, 0)], [(0, 1)], [(0, 2), (1, 2), (2, 2)]]),
        E((R.ADD, 0, 3, 4), (R.REPLACE, 1, 0), (R.REPLACE, 0, 2)))
    add("two_new_points_on_one_idx2", w([[(0, 0)], [], []]),
        E((R.SET_REF, 1, 4), (R.ADD, 1, 4, 1), (R.ADD, 1, 2, 6), (R.SET_REF, 2, 4), (R.ADD, 2, 4, 2), (R.ADD, 2, 2, 6)))
    a = w([[(0, 0), (1, 0)], [(2, 1)]], slots={(4, 1): 0, (4, 5): 0, (4, 2): 1})
    import pilotguru_amd.map_edit as M
    add("point_in_two_slots_of_a_new_key_frame", a, M.map_edits_from_keyframe(a["kf_point"][4], 2, a["point_bad"], a["obs_start"], a["obs_frame"], a["obs_live"], 4)[0]
        .astype(R.EDIT_DTYPE))
    add("dead_masked_input", w([[(0, 0), (1, 0, 0), (2, 0)], [(3, 1, 0), (4, 1), (0, 1, 0)], [(1, 2), (2, 2, 0)]], ref={0: 1, 1: 4, 2: 1}), E((R.ADD, 0, 1, 4)))
    add("bad_indices", w([[(0, 0)], [(1, 1)]]),
        E((R.ADD, 2, 0, 0), (R.ADD, 0, 5, 0), (R.ADD, 0, 1, 8), (R.ADD, 0, 1, -1), (R.REPLACE, 0, 2), (R.REPLACE, -1, 0), (R.ERASE, 0, -1), (R.SET_REF, 0, 5),
          (R.ADD, 0, 1, 7)))
    add("selection_of_survivors_only", w([[(0, 0)], [(1, 1)], [(2, 2)]]), E((R.REPLACE, 0, 1), (R.ADD, 2, 3, 3)), select_bits=R.TOUCH_SURVIVOR)
    add("stale_descriptor", w([[(0, 0)], [(1, 1)], [(2, 2)]]), E((R.REPLACE, 0, 1), (R.ADD, 1, 3, 3)))
    add("empty_edit_list_compacts", w([[(0, 0), (1, 0, 0), (2, 0)], [(3, 1, 0)]], ref={0: 2}), E())
    return out


def padded(c, seed=0):
    """the same edits with NOPs in between"""
    r = np.random.RandomState(seed)
    rows = []
    for e in c.edits:
        rows += [(R.NOP, 9, 9, 9)] * r.randint(0, 3) + [tuple(e)]
    rows += [(R.NOP, 0, 0, 0)] * 2
    ed = E(*rows)
    return Case(c.name + "_padded", c.a, ed, c.obs_cap_out, c.select_bits, c.sel_cap), np.array([k for k, x in enumerate(ed) if x["op"] != R.NOP], int)


def random_world(seed):
    r = np.random.RandomState(1000 + seed)
    nkf = r.randint(4, 13)
    nslots = r.randint(6, 17)
    npoints = r.randint(6, 49)
    order = r.permutation(nkf)
    free = {f: list(r.permutation(nslots)) for f in range(nkf)}
    lists, bad = [], []
    for p in range(npoints):
        k = r.choice([0, 1, 2, 3, 3, 4, 4, 5, 6])
        lst = []
        for f in r.permutation(nkf)[:min(k, nkf)]:
            if free[f]:
                lst.append((int(f), int(free[f].pop()), int(r.rand() > 0.1)))
        if r.rand() < 0.08:
            bad.append(p)
        lists.append(lst)
    slots = {}
    for _ in range(r.randint(0, 4)):                          # dangling: a slot that holds another point than the one that lists it
        slots[(int(r.randint(nkf)), int(r.randint(nslots)))] = int(r.randint(-1, npoints))
    ref = {}
    for p, lst in enumerate(lists):
        if lst and r.rand() < 0.9:
            ref[p] = lst[r.randint(len(lst))][0]
    a = world(nkf, nslots, lists, order, bad=bad, ref=ref, slots=slots, visible=r.randint(1, 50, npoints), found=r.randint(0, 30, npoints))
    ne = r.randint(1, 65)
    rows = []
    hot = r.choice(npoints, min(npoints, r.randint(2, 9)), replace=False)     # edits gather on a few points, so that components form
    pick = lambda: int(hot[r.randint(len(hot))]) if r.rand() < 0.7 else int(r.randint(npoints))
    for _ in range(ne):
        u = r.rand()
        p = pick()
        if u < 0.1:
            rows.append((R.NOP, 0, 0, 0))
        elif u < 0.4:
            rows.append((R.ADD, p, int(r.randint(nkf)), int(r.randint(nslots))))
        elif u < 0.65:
            rows.append((R.REPLACE, p, pick(), 0))
        elif u < 0.93:
            lst = lists[p]
            rows.append((R.ERASE, p, int(lst[r.randint(len(lst))][0]) if lst and r.rand() < 0.85 else int(r.randint(nkf)), 0))
        elif u < 0.97:
            rows.append((R.SET_REF, p, int(r.randint(nkf)), 0))
        else:
            rows.append((int(r.choice([R.ADD, R.REPLACE, R.ERASE])), int(r.randint(-1, npoints + 2)), int(r.randint(-1, nkf + 2)), int(r.randint(-1, nslots + 1))))
    return Case("random%d" % seed, a, E(*rows))


def sentinel(c, extra=2):
    a = c.a
    npoints, ne = len(a["obs_start"]) - 1, len(c.edits)
    cap_out = c.obs_cap_out if c.obs_cap_out is not None else int(a["obs_live"].sum()) + int(np.sum(c.edits["op"] == R.ADD))
    sel_cap = npoints if c.sel_cap is None else c.sel_cap
    full = lambda k: np.full(k + extra, SENT, np.int32)
    return cap_out, sel_cap, dict(obs_start_out=full(npoints + 1), obs_frame_out=full(cap_out), obs_idx_out=full(cap_out), ref_obs_out=full(npoints),
                                  edit_status=full(ne), touched=full(npoints), select_out=full(sel_cap), info=full(R.INFO))


def expected(c, rules=None, exact=True):
    """what the reference leaves.  obs_cap_out None: the reference's own new length (exact) -- or live + ADDs, the room a caller gives"""
    cap_out, sel_cap, s = sentinel(c)
    if c.obs_cap_out is None and exact:
        probe = R.apply_edits(c.a, c.edits, cap_out, c.select_bits, sel_cap, rules)      # live + ADDs bounds the new length
        cap_out = int(probe["info"][1]) if probe["info"][0] != R.LIMIT else cap_out
        c2 = dataclasses.replace(c, obs_cap_out=cap_out)
        cap_out, sel_cap, s = sentinel(c2)
    e = R.apply_edits(c.a, c.edits, cap_out, c.select_bits, sel_cap, rules, s)
    e["obs_cap_out"], e["sel_cap"] = cap_out, sel_cap
    return e


def same(x, y):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in KEYS)


def diff(x, y):
    return [k for k in KEYS if not np.array_equal(np.asarray(x[k]), np.asarray(y[k]))]


# ---------------------------------------------------------------- the decomposition, as the kernels carry it out
def apply_decomposed(c, e):
    """components by min-propagation, a stable bucket, one bag per component walked in edit order with the last write per slot,
    every result in scratch; then the limit decision; then the commit, slots by the largest edit index.  e: expected() for the
    capacities and the sentinel."""
    a, edits = c.a, c.edits
    n, cap, nkf = a["n"], a["cap"], len(a["n"])
    rank = a["order"] if a["order"] is not None else np.arange(nkf)
    npoints, ne = len(a["obs_start"]) - 1, len(edits)
    st, of, oi, lv = a["obs_start"], a["obs_frame"], a["obs_idx"], a["obs_live"]
    valid = np.array([x["op"] != R.NOP and R.edit_valid(a, x) for x in edits], bool)
    # k_edit_init
    live_list = lambda p: [(int(of[o]), int(oi[o])) for o in range(st[p], st[p + 1]) if lv[o]]
    sBad, sVis, sFound, sRepl = a["point_bad"].astype(np.int32), a["visible"].copy(), a["found"].copy(), a["replaced"].copy()
    sRef = np.full(npoints, -1, np.int32)
    for p in range(npoints):
        ro = int(a["ref_obs"][p])
        if 0 <= ro < st[p + 1] - st[p] and lv[st[p] + ro]:
            sRef[p] = of[st[p] + ro]
    touched, new_len = np.zeros(npoints, np.int32), np.array([len(live_list(p)) for p in range(npoints)], np.int32)
    loaded, final = np.zeros(npoints, bool), {}
    status = np.where(valid | (edits["op"] == R.NOP), 0, R.BAD_INDEX).astype(np.int32)
    # k_edit_components: the label of a point only falls, until no REPLACE pair disagrees
    comp = np.arange(npoints)
    while True:
        changed = False
        for k in np.nonzero(valid & (edits["op"] == R.REPLACE))[0]:
            x, y = int(edits["a"][k]), int(edits["b"][k])
            m = min(comp[x], comp[y])
            if comp[x] != m or comp[y] != m:
                comp[x] = comp[y] = m
                changed = True
        if not changed:
            break
    # k_edit_bucket: stable by (component, position)
    idx = np.nonzero(valid)[0]
    idx = idx[np.argsort(comp[edits["a"][idx]], kind="stable")]
    groups = {}
    for k in idx:
        groups.setdefault(int(comp[edits["a"][k]]), []).append(int(k))
    records, limit, applied, writes = [], int(valid.sum()) > R.MAX_EDITS, 0, 0         # k_edit_bucket: more than the sort holds
    if limit:
        groups = {}
    # k_edit_plan
    for root in sorted(groups):
        bag, pend, used = [], {}, 0                            # bag: [point, key frame, keypoint] with point -1 = killed; pend: slot -> (value, edit)

        def load(p):
            nonlocal used
            if not loaded[p]:
                for f, i in live_list(p):
                    bag.append([p, f, i])
                used += len(live_list(p))
                loaded[p] = True
                new_len[p] = 0

        def changed_(p):
            touched[p] |= R.TOUCH_CHANGED | (R.TOUCH_STALE if touched[p] & R.TOUCH_SURVIVOR else 0)
        for k in groups[root]:
            op, x, y, z = (int(v) for v in edits[k])
            s = R.APPLIED
            if op == R.ADD:
                load(x)
                used += 1
                if used > R.MAX_BAG:
                    limit = True
                    break
                if not any(t[0] == x and t[1] == y for t in bag):
                    bag.append([x, y, z])
                    changed_(x)
                else:
                    s |= R.ALREADY
                pend[y * cap + z] = (x, k)
                writes += 1
            elif op == R.REPLACE:
                if x == y:
                    s = R.SELF
                else:
                    load(x)
                    load(y)
                    if used > R.MAX_BAG:
                        limit = True
                        break
                    mine = [t for t in bag if t[0] == x]
                    gained = 0
                    for t in mine:
                        has = any(u[0] == y and u[1] == t[1] for u in bag)
                        pend[t[1] * cap + t[2]] = (-1 if has else y, k)
                        t[0] = -1 if has else y
                        gained += not has
                    writes += len(mine)
                    if mine:
                        touched[x] |= R.TOUCH_CHANGED
                    sBad[x], sRepl[x] = 1, y
                    sFound[y] = R._i32(int(sFound[y]) + int(sFound[x]))
                    sVis[y] = R._i32(int(sVis[y]) + int(sVis[x]))
                    if gained:
                        touched[y] |= R.TOUCH_CHANGED
                    touched[y] = (touched[y] | R.TOUCH_SURVIVOR) & ~R.TOUCH_STALE
            elif op == R.ERASE:
                load(x)
                if used > R.MAX_BAG:
                    limit = True
                    break
                hit = [t for t in bag if t[0] == x and t[1] == y]
                if not hit:
                    s = R.NOT_OBSERVED
                else:
                    pend[y * cap + hit[0][2]] = (-1, k)
                    writes += 1
                    hit[0][0] = -1
                    changed_(x)
                    left = [t for t in bag if t[0] == x]
                    if sRef[x] == y:
                        sRef[x] = min(left, key=lambda t: (rank[t[1]], t[1]))[1] if left else -1
                    if len(left) <= 2:
                        s |= R.WENT_BAD
                        sBad[x] = 1
                        for t in left:
                            pend[t[1] * cap + t[2]] = (-1, k)
                            writes += 1
                            t[0] = -1
            else:
                sRef[x] = y
            status[k] = s
            applied += bool(s & R.APPLIED)
        if limit:
            break
        records += [(slot, v, k) for slot, (v, k) in pend.items()]
        for t in sorted([t for t in bag if t[0] >= 0], key=lambda t: (t[0], rank[t[1]], t[1])):
            final.setdefault(t[0], []).append((t[1], t[2]))
            new_len[t[0]] += 1
    # k_edit_scan: the limit decision before any output byte
    out = {k: np.array(v) for k, v in e.items() if k in KEYS}
    out.update({k: a[k].copy() for k in ("kf_point", "point_bad", "visible", "found", "replaced")})
    _, _, s0 = sentinel(dataclasses.replace(c, obs_cap_out=e["obs_cap_out"], sel_cap=e["sel_cap"]))
    out.update({k: v for k, v in s0.items()})
    sel = [p for p in range(npoints) if e["sel_cap"] and touched[p] & c.select_bits]
    total = int(new_len.sum())
    if limit or total > e["obs_cap_out"] or len(sel) > e["sel_cap"]:
        out["info"][0] = R.LIMIT
        return out
    # k_edit_mark, k_edit_commit
    slots = out["kf_point"].reshape(-1)
    mark = {}
    for slot, v, k in records:
        mark[slot] = max(mark.get(slot, -1), k)
    for slot, v, k in records:
        if mark[slot] == k:
            slots[slot] = v
    start = np.concatenate([[0], np.cumsum(new_len)]).astype(np.int32)
    out["obs_start_out"][:npoints + 1] = start
    for p in range(npoints):
        lst = final.get(p, []) if loaded[p] else live_list(p)
        for k, (f, i) in enumerate(lst):
            out["obs_frame_out"][start[p] + k], out["obs_idx_out"][start[p] + k] = f, i
        out["ref_obs_out"][p] = next((k for k, (f, _) in enumerate(lst) if f == sRef[p]), -1)
    out["point_bad"], out["visible"], out["found"], out["replaced"] = (sBad != 0).astype(np.uint8), sVis, sFound, sRepl
    out["edit_status"][:ne] = status
    out["touched"][:npoints] = touched
    out["select_out"][:e["sel_cap"]] = -1
    out["select_out"][:len(sel)] = sel
    out["info"][:R.INFO] = [0, total, applied, int(np.sum((sBad != 0) & (a["point_bad"] == 0))), len(groups), writes, int(np.sum((touched & R.TOUCH_STALE) != 0)), len(sel)]
    return out


# ---------------------------------------------------------------- the device and host forms
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def upload(c, e):
    a = c.a
    one = lambda x, dt: x if len(x) else np.zeros(1, dt)
    d = {k: dev(a[k]) for k in ("n", "kf_point", "point_bad", "visible", "found", "replaced", "obs_start", "ref_obs")}
    d.update(order=None if a["order"] is None else dev(a["order"]), obs_frame=dev(one(a["obs_frame"], np.int32)), obs_idx=dev(one(a["obs_idx"], np.int32)),
             obs_live=dev(one(a["obs_live"], np.uint8)), edits=dev(np.frombuffer(one(c.edits, R.EDIT_DTYPE).tobytes(), np.int32).copy()))
    _, _, s = sentinel(dataclasses.replace(c, obs_cap_out=e["obs_cap_out"], sel_cap=e["sel_cap"]))
    d.update({k: dev(v) for k, v in s.items()})
    return d


def run_device(c, ext, e, stream=None, d=None, nedits_dev=None, live=True):
    import torch
    a = c.a
    d = d or upload(c, e)
    s = stream if stream is not None else torch.cuda.current_stream()
    rc = ext._L.pgorb_apply_map_edits_device(
        ext._h, ptr(d["edits"]), len(c.edits), ptr(nedits_dev), ptr(d["kf_point"]), ptr(d["n"]), len(a["n"]), a["cap"], ptr(d["order"]),
        len(a["obs_start"]) - 1, ptr(d["point_bad"]), ptr(d["visible"]), ptr(d["found"]), ptr(d["replaced"]), ptr(d["obs_start"]), ptr(d["obs_frame"]),
        ptr(d["obs_idx"]), a["nobs"], ptr(d["obs_live"]) if live else None, ptr(d["ref_obs"]), e["obs_cap_out"], ptr(d["obs_start_out"]),
        ptr(d["obs_frame_out"]), ptr(d["obs_idx_out"]), ptr(d["ref_obs_out"]), ptr(d["edit_status"]), ptr(d["touched"]), c.select_bits, e["sel_cap"],
        ptr(d["select_out"]), ptr(d["info"]), C.c_void_p(s.cuda_stream))
    assert rc == 0, (rc, ext._L.pgorb_last_error(ext._h))
    return d


def download(d):
    import torch
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in KEYS}


def run_host(c, ext, e):
    """pgorb_apply_map_edits on copies; raises AssertionError((rc, message)) for a refusal"""
    a = c.a
    nkf, npoints, ne = len(a["n"]), len(a["obs_start"]) - 1, len(c.edits)
    slots = [a["kf_point"][f, :a["n"][f]].copy() for f in range(nkf)]
    ptrs = (C.c_void_p * max(nkf, 1))()
    for f, s in enumerate(slots):
        ptrs[f] = s.ctypes.data if len(s) else None
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    one = lambda x, dt: x if len(x) else np.zeros(1, dt)
    io = {k: a[k].copy() for k in ("point_bad", "visible", "found", "replaced")}
    _, _, s = sentinel(dataclasses.replace(c, obs_cap_out=e["obs_cap_out"], sel_cap=e["sel_cap"]))
    ed, of, oi, lv = one(c.edits, R.EDIT_DTYPE), one(a["obs_frame"], np.int32), one(a["obs_idx"], np.int32), one(a["obs_live"], np.uint8)
    rc = ext._L.pgorb_apply_map_edits(
        ext._h, p(ed), ne, nkf, ptrs, p(a["n"]), p(a["order"]), npoints, p(io["point_bad"]), p(io["visible"]), p(io["found"]), p(io["replaced"]),
        p(a["obs_start"]), p(of), p(oi), p(lv), p(a["ref_obs"]), e["obs_cap_out"], p(s["obs_start_out"]), p(s["obs_frame_out"]), p(s["obs_idx_out"]),
        p(s["ref_obs_out"]), p(s["edit_status"]), p(s["touched"]), c.select_bits, e["sel_cap"], p(s["select_out"]), p(s["info"]))
    assert rc >= 0, (rc, ext._L.pgorb_last_error(ext._h))
    kf_point = a["kf_point"].copy()
    for f in range(nkf):
        kf_point[f, :a["n"][f]] = slots[f]
    out = dict(io, kf_point=kf_point, **s)
    out["returned"] = rc
    return out
