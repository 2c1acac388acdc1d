"""TEST INFRASTRUCTURE ONLY — the labelling chain in two halves (ssdr_oracle_label_verdict_dev / ssdr_oracle_label_walk_dev) with the ranks of a
sharded round emulated in one process: the clouds are split into contiguous shares, every "rank" judges its own picks into its slice of ONE record
buffer (what the all-gather of the sharded round produces) and then walks all records over its own pseudo-label arrays.  The reference is the one-call
chain ssdr_oracle_label_dev over the union of the clouds, itself pinned to _labeling_oracle.label_round."""
import ctypes as C

import numpy as np

import _labeling_oracle as O

RECORD_BYTES = 80
DEAD = np.uint64(0xffffffffffffffff)
MODES = {"dominant": 0, "NAIL": 1}


def split_clouds(n_clouds, world, empty_rank=None):
    """contiguous shares of the clouds, rank by rank (a rank of `empty_rank` still owns clouds: it only receives no pick)"""
    return [list(x) for x in np.array_split(np.arange(n_clouds), world)]


def walk_keys(picks, owner, cloud_key=None):
    """per rank: the slots' global pick positions and their 64-bit keys.  cloud_key None: first appearance of the cloud among ALL picks in the high half,
    the global pick position in the low half (fps / k-center); else cloud_key[cloud] and the position among the rank's own picks (edcd / topk)."""
    first = {}
    for i, (c, _) in enumerate(picks):
        first.setdefault(c, i)
    out = []
    for r in range(max(owner) + 1):
        mine = [i for i, (c, _) in enumerate(picks) if owner[c] == r]
        hi = [first[picks[i][0]] if cloud_key is None else int(cloud_key[picks[i][0]]) for i in mine]
        lo = mine if cloud_key is None else list(range(len(mine)))
        out.append((np.asarray(mine, np.int64), np.asarray([(h << 32) | l for h, l in zip(hi, lo)], np.uint64)))
    return out


class Sharded:
    """the device arrays of every emulated rank over its share of `clouds`; records = one buffer of world * max_items records"""

    def __init__(self, clouds, shares, picks, max_items, cloud_key=None, labeled=None, pseudo=None):
        from ssdr_al._lib import DevArray
        self.clouds, self.shares, self.picks, self.W, self.M = clouds, shares, picks, len(shares), int(max_items)
        self.owner = {c: r for r, sh in enumerate(shares) for c in sh}
        self.keys = walk_keys(picks, self.owner, cloud_key)
        self.rec = DevArray.from_host(np.full(self.W * max(self.M, 1) * RECORD_BYTES, 0xAB, np.uint8))
        self.ranks = []
        ubase = np.concatenate([[0], np.cumsum([len(c["components"]) for c in clouds])]).astype(np.int64)
        up0 = np.concatenate([[0], np.cumsum([len(c["gt"]) for c in clouds])]).astype(np.int64)
        for r, sh in enumerate(shares):
            gt, pred, off, pts, _, base, p0 = O.concat_clouds([clouds[c] for c in sh])
            where = {c: k for k, c in enumerate(sh)}
            mine, keys = self.keys[r]
            items = np.array([base[where[picks[i][0]]] + picks[i][1] for i in mine] + [0], np.int32)
            s_lo, s_hi, p_lo, p_hi = int(ubase[sh[0]]), int(ubase[sh[-1] + 1]), int(up0[sh[0]]), int(up0[sh[-1] + 1])
            ps = np.zeros((2, len(gt)), np.float32) if pseudo is None else np.asarray(pseudo[:, p_lo:p_hi], np.float32)
            lab = np.zeros(len(off) - 1, np.uint8) if labeled is None else labeled[s_lo:s_hi].astype(np.uint8)
            self.ranks.append(dict(
                n=len(gt), S=len(off) - 1, n_items=len(mine), max_region=int(np.diff(off).max()), mine=mine,
                gt=DevArray.from_host(gt), pred=DevArray.from_host(pred), off=DevArray.from_host(off), pts=DevArray.from_host(pts),
                items=DevArray.from_host(items), cnt=DevArray.from_host(np.array([len(mine)], np.int32)),
                keys=DevArray.from_host(np.concatenate([keys, [0]]).astype(np.uint64)), pseudo0=ps, labeled0=lab))

    def verdicts(self, mode, thr, min_size, nl=13, nc=13, max_region=None):
        """the verdict half of every rank into its slice of the record buffer; -> the return codes"""
        from ssdr_al import _lib
        L = _lib.lib()
        rcs = []
        for r, R in enumerate(self.ranks):
            rcs.append(L.ssdr_oracle_label_verdict_dev(R["gt"].ptr, R["pred"].ptr, R["n"], R["off"].ptr, R["pts"].ptr, R["S"], R["items"].ptr, R["cnt"].ptr, self.M,
                                                       R["keys"].ptr, R["max_region"] if max_region is None else max_region, nl, nc, MODES.get(mode, 9), thr, min_size,
                                                       self.rec.ptr + r * self.M * RECORD_BYTES, None))
        _lib.sync()
        return rcs

    def records(self):
        dt = np.dtype([("key", "<u8"), ("pos", "<i4"), ("kind", "<i4"), ("lab", "<i4"), ("cost", "<i4"), ("nent", "<i4"), ("subp", "<i4"), ("len", "<i4"),
                       ("smask", "<u4"), ("sublab", "u1", 32), ("status", "<i4"), ("pad", "<i4")])
        assert dt.itemsize == RECORD_BYTES
        return self.rec.to_host()[: self.W * self.M * RECORD_BYTES].view(dt).reshape(self.W, self.M)

    def walk(self, budget, nc=13, class_cap=None, max_region=None):
        """the walk half of every rank over the whole record buffer; -> per rank dict(rc, out, pseudo, used, labeled, classes, budget, walk_pos)"""
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        L = _lib.lib()
        cap = max(1, self.W * self.M * 32) if class_cap is None else class_cap
        res = []
        for r, R in enumerate(self.ranks):
            d = dict(budget=DevArray.from_host(np.array([budget], np.int64)), mask=DevArray.from_host(np.ascontiguousarray(R["pseudo0"][0])),
                     label=DevArray.from_host(np.ascontiguousarray(R["pseudo0"][1])), used=DevArray.from_host(np.full(max(self.M, 1), 7, np.uint8)),
                     labeled=DevArray.from_host(R["labeled0"]), cls=DevArray.from_host(np.full(cap + 1, -5, np.int32)),
                     pos=DevArray.from_host(np.full(max(self.M, 1), -7, np.int32)), out=DevArray.from_host(np.full(12, -9, np.int64)))
            rc = L.ssdr_oracle_label_walk_dev(self.rec.ptr, r, self.W, R["pred"].ptr, R["n"], R["off"].ptr, R["pts"].ptr, R["S"], R["items"].ptr, R["cnt"].ptr, self.M,
                                              R["max_region"] if max_region is None else max_region, nc, d["budget"].ptr, d["mask"].ptr, d["label"].ptr, d["used"].ptr,
                                              d["labeled"].ptr, d["cls"].ptr, cap, d["pos"].ptr, d["out"].ptr, None)
            if rc:
                res.append(dict(rc=rc))
                continue
            _lib.sync()
            out, cls = d["out"].to_host(), d["cls"].to_host()
            assert cls[cap] == -5                                             # nothing behind the class list's capacity
            res.append(dict(rc=0, out=out, pseudo=np.stack([d["mask"].to_host(), d["label"].to_host()]), used=d["used"].to_host()[: self.M],
                            labeled=d["labeled"].to_host() != 0, classes=cls[: min(int(out[6]), cap)].tolist(), cls_raw=cls, budget=int(d["budget"].to_host()[0]),
                            walk_pos=d["pos"].to_host()[: self.M]))
        return res

    def merged(self, res):
        """the ranks' results as the one-call chain lays them out: pseudo labels and labelled mask over the union, used flags and walk positions by
        global pick position"""
        n = len(self.picks)
        used, pos = np.zeros(n, np.uint8), np.full(n, -1, np.int64)
        for R, x in zip(self.ranks, res):
            k = R["n_items"]
            used[R["mine"]] = x["used"][:k]; pos[R["mine"]] = x["walk_pos"][:k]
            assert not x["used"][k:].any() and (x["walk_pos"][k:] == -1).all()      # dead slots: neither used nor in the walk
        return dict(pseudo=np.concatenate([x["pseudo"] for x in res], axis=1), labeled=np.concatenate([x["labeled"] for x in res]), used=used, walk_pos=pos)


def one_call(clouds, picks, mode, thr, budget, min_size, nl=13, nc=13, cloud_key=None, class_cap=None, labeled=None, pseudo=None, max_region=None):
    """ssdr_oracle_label_dev over the union of the clouds (the reference of the two halves)"""
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    gt, pred, off, pts, cloud, base, p0 = O.concat_clouds(clouds)
    n, S, M = len(gt), len(off) - 1, len(picks)
    items = np.array([base[c] + s for c, s in picks] + [0], np.int32)
    ps = np.zeros((2, n), np.float32) if pseudo is None else np.asarray(pseudo, np.float32)
    cap = max(1, M * 32) if class_cap is None else class_cap
    d = dict(gt=DevArray.from_host(gt), pred=DevArray.from_host(pred), off=DevArray.from_host(off), pts=DevArray.from_host(pts), cloud=DevArray.from_host(cloud),
             items=DevArray.from_host(items), n=DevArray.from_host(np.array([M], np.int32)), budget=DevArray.from_host(np.array([budget], np.int64)),
             mask=DevArray.from_host(np.ascontiguousarray(ps[0])), label=DevArray.from_host(np.ascontiguousarray(ps[1])), used=DevArray.from_host(np.full(max(M, 1), 7, np.uint8)),
             labeled=DevArray.from_host(np.zeros(S, np.uint8) if labeled is None else labeled.astype(np.uint8)), cls=DevArray.from_host(np.full(cap + 1, -5, np.int32)),
             proc=DevArray((max(M, 1),), np.int32), out=DevArray((12,), np.int64))
    d_key = None if cloud_key is None else DevArray.from_host(np.asarray(cloud_key, np.int32))
    rc = _lib.lib().ssdr_oracle_label_dev(d["gt"].ptr, d["pred"].ptr, n, d["off"].ptr, d["pts"].ptr, S, d["cloud"].ptr, len(clouds), d["items"].ptr, d["n"].ptr, M,
                                          None if d_key is None else d_key.ptr, int(np.diff(off).max()) if max_region is None else max_region, nl, nc, MODES[mode], thr,
                                          min_size, d["budget"].ptr, d["mask"].ptr, d["label"].ptr, d["used"].ptr, d["labeled"].ptr, d["cls"].ptr, cap, d["proc"].ptr,
                                          d["out"].ptr, None)
    assert rc == 0
    _lib.sync()
    out, cls = d["out"].to_host(), d["cls"].to_host()
    return dict(out=out, pseudo=np.stack([d["mask"].to_host(), d["label"].to_host()]), used=d["used"].to_host()[:M], proc=d["proc"].to_host()[:M],
                labeled=d["labeled"].to_host() != 0, classes=cls[: min(int(out[6]), cap)].tolist(), cls_raw=cls, budget=int(d["budget"].to_host()[0]), base=base)


def assert_halves_equal_one_call(sh, res, ref):
    """every comparison is exact: the union of the ranks' points / used flags / labelled masks, the class list, d_out[0..11] and the budget on every rank,
    and the walk positions against d_proc_order"""
    m = sh.merged(res)
    assert np.array_equal(m["pseudo"], ref["pseudo"])
    assert np.array_equal(m["used"], ref["used"]) and np.array_equal(m["labeled"], ref["labeled"])
    for x in res:
        assert x["rc"] == 0 and x["out"].tolist() == ref["out"].tolist()
        assert x["classes"] == ref["classes"] and x["budget"] == ref["budget"] == int(ref["out"][7])
        assert np.array_equal(x["cls_raw"][: len(ref["cls_raw"])], ref["cls_raw"][: len(x["cls_raw"])])
    at = m["walk_pos"]
    reached = np.flatnonzero(at >= 0)
    assert sorted(at[reached].tolist()) == list(range(len(reached)))          # the walk reaches a prefix of the order, every position once
    assert np.array_equal(ref["proc"][at[reached]], reached)
    assert not m["used"][at < 0].any()
    return m


def walk_costs(clouds, picks, mode, thr, min_size, cloud_order=None):
    """the walk order [(cloud, region)] and what every item costs when the budget reaches it, from the NumPy oracle alone"""
    order = [(c, s) for c, sps in O.help_order(picks, cloud_order) for s in sps]
    cache, costs = {}, []
    for c, s in order:
        if (c, s) not in cache:
            b = {"click": 1 << 30}
            O.oracle_labeling([s], clouds[c]["components"], np.asarray(clouds[c]["gt"]), np.zeros((2, len(clouds[c]["gt"])), np.float32), dict.fromkeys(O.COUNTERS, 0),
                              mode, clouds[c]["pred"], thr, b, min_size, [])
            cache[(c, s)] = (1 << 30) - b["click"]
        costs.append(cache[(c, s)])
    return order, np.asarray(costs, np.int64)
