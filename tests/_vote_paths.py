"""Helpers of tests/test_vote_paths.py: the constants of the vote / feed generator read from csrc/vote.hip, the caps its launchers write as plain literals, the
predictors of the branch a call takes (`sort_path`, `rstride`, `vm_grid`, `init_grid`; the threshold bin, the candidates and the sort ranges come from
_tile_paths.plan, which describes vote_thresh too once the shared constants are seen to be equal), tables of clouds, draws, the oracle stepped tile by tile
(_feed_oracle.ChainGenerator / indep_batch, unchanged), and the callers of ssdr_vote_init_dev / ssdr_vote_tiles_dev / ssdr_feed_chain_dev / ssdr_feed_tiles_dev /
ssdr_feed_status.  Nothing here touches a device except `Table` and `feed_status`.

A table (`make_table`) is a SimpleNamespace: clouds (dicts xyz float32 [n, 3], rgb uint8 [n, 3], labels int32 [n], as _vote_oracle.make_case makes them), acts /
pses (float32 [n] each), off (int64 row offsets).  Draws (`make_draws`) are the dict of _vote_oracle.draw_batch: noise float32 [B, 3], perm int32 [B, N], dup
float32 [B, N] with dup_u = 0 in the row before the last and 1.0 in the last of every tile."""
import os
import re
from types import SimpleNamespace

import numpy as np

import _feed_oracle as FO
import _tile_paths as TP
from _tile_paths import F32, SENTINEL_F, SENTINEL_I
from conftest import assert_bits_equal

SCALE = F32(1.0 / 255.0)
XY_ONLY, GLOBAL_ROWS = 1, 2                       # SSDR_FEED_XY_ONLY, SSDR_FEED_GLOBAL_ROWS (include/ssdr_al.h)
ST_LABEL, ST_CLOUD, ST_POINT = 1, 2, 4            # the bits of ssdr_feed_status
ERR_INVALID = 1
MAX_CLOUDS = 4096                                 # VOTE_MAX_CLOUDS

# caps the launchers of csrc/vote.hip write as plain literals
SORT_GRID_CAP = 64                                # vote_chain_launch / vote_indep_launch: vote_sort's grid, dim3(std::min(rstride, 64))
INIT_GRID_CAP = 64                                # ssdr_vote_init_dev: const int gx = std::min(vm_grid(maxn), 64)
COMPACT_GRID_CAP = 256                            # both launchers: g_comp = std::max(1, std::min((maxn + 256 * TS_CPT - 1) / (256 * TS_CPT), 256))
HIST_GRID_CAP = 64                                # both launchers: g_hist = std::max(1, std::min((maxn + 255) / 256, 64))
BLOCK = 256                                       # every kernel's workgroup; vote_pick's `c += 256`, vote_place's tiles per workgroup


# ---- constants, from the source -------------------------------------------------------------------------------------------------------------------
_CONSTANTS = None


def constants():
    """TS_BITS, TS_RSTEP, TS_RCAP, TS_RMAX, TS_CPT, VM_CHUNK, VM_MAXPART of csrc/vote.hip, one definition each; the four it shares with csrc/tile.hip are equal there,
    so _tile_paths.plan (bins, threshold, ranges) holds for vote_hist / vote_thresh as it stands"""
    global _CONSTANTS
    if _CONSTANTS is None:
        path = os.path.join(TP.CSRC, "vote.hip")
        with open(path) as f:
            text = f.read()
        out = {}
        for nm in ("TS_BITS", "TS_RSTEP", "TS_RCAP", "TS_RMAX", "TS_CPT", "VM_CHUNK", "VM_MAXPART"):
            m = re.findall(r"\b%s\s*=\s*([0-9]+)\s*[,;]" % nm, text)
            assert len(m) == 1, "%s: expected one definition of %s, found %d" % (path, nm, len(m))
            out[nm] = int(m[0])
        tile = TP.constants()
        for nm in ("TS_BITS", "TS_RSTEP", "TS_RCAP", "TS_RMAX"):
            assert out[nm] == getattr(tile, nm), "%s: %d in vote.hip, %d in tile.hip" % (nm, out[nm], getattr(tile, nm))
        _CONSTANTS = SimpleNamespace(**out)
    return _CONSTANTS


# ---- predictors ---------------------------------------------------------------------------------------------------------------------------------------
def sort_path(n):
    """the branch of vote_sort a range of n words takes (no register form here)"""
    if n <= 1:
        return "none"
    return "lds" if n <= constants().TS_RCAP else "global"


def rstride(maxn):
    """the range-table stride of a call over a table whose largest cloud has maxn rows; above TS_RMAX the call takes vote_compact_bins"""
    k = constants()
    return (maxn + k.TS_RSTEP - 1) // k.TS_RSTEP + 1


def vm_grid(maxn):
    """vote_min_part's grid in the chain: one workgroup per VM_CHUNK rows of the largest cloud, at most VM_MAXPART"""
    k = constants()
    return max(1, min((maxn + k.VM_CHUNK - 1) // k.VM_CHUNK, k.VM_MAXPART))


def init_grid(maxn):
    """vote_min_part's grid x in ssdr_vote_init_dev"""
    return min(vm_grid(maxn), INIT_GRID_CAP)


def chunks(n):
    return (n + constants().VM_CHUNK - 1) // constants().VM_CHUNK


def compact_passes(maxn):
    """the trips of vote_compact's loop a workgroup takes over the largest cloud"""
    per = BLOCK * constants().TS_CPT
    g = max(1, min((maxn + per - 1) // per, COMPACT_GRID_CAP))
    return ((maxn + per - 1) // per + g - 1) // g


def tile_plans(table, ref, N):
    """_tile_paths.plan of every tile of an oracle batch (its cloud, its centre), with dmax: the largest key among the tile's rows"""
    out = []
    for c, centre in zip(ref["cloud"], ref["center"]):
        pts = table.clouds[int(c)]["xyz"]
        p = TP.plan(pts, centre, N, len(pts))
        p.dmax = np.sort(TP.keys(pts, centre))[min(N, len(pts)) - 1]
        out.append(p)
    return out


def assert_update_defined(plans):
    """a chain tile whose largest key is 0 or inf makes the reference's own update NaN: out of scope, and the cases avoid it"""
    for t, p in enumerate(plans):
        assert np.isfinite(p.dmax) and p.dmax > 0, "tile %d: dmax %r" % (t, p.dmax)


# ---- tables, draws --------------------------------------------------------------------------------------------------------------------------------------
def make_table(rng, xyzs, num_labels=8):
    clouds, acts, pses = [], [], []
    for p in xyzs:
        n = len(p)
        clouds.append(dict(xyz=np.ascontiguousarray(p, F32), rgb=rng.integers(0, 256, (n, 3)).astype(np.uint8), labels=rng.integers(0, num_labels, n).astype(np.int32)))
        acts.append((rng.random(n) < 0.3).astype(F32))
        pses.append(rng.integers(0, 8, n).astype(F32))
    off = np.concatenate([[0], np.cumsum([len(p) for p in xyzs])]).astype(np.int64)
    return SimpleNamespace(clouds=clouds, acts=acts, pses=pses, off=off, sizes=[len(p) for p in xyzs], maxn=max(len(p) for p in xyzs))


def make_draws(rng, B, N, noise_scale=0.35):
    dup = rng.random((B, N)).astype(F32)
    dup[:, -1] = 1.0
    if N > 1:
        dup[:, -2] = 0.0
    return dict(noise=rng.normal(scale=noise_scale, size=(B, 3)).astype(F32), perm=np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32), dup=dup)


def towards(table, cloud, point, centre):
    """the noise that puts a tile's centre on `centre`; exact for the origin: x + (-x) = 0"""
    return (np.asarray(centre, F32) - table.clouds[cloud]["xyz"][point]).astype(F32)


# ---- oracles, stepped -----------------------------------------------------------------------------------------------------------------------------------
def chain_oracle(table, poss, N, flags=GLOBAL_ROWS, weights=None, channels=True):
    """_feed_oracle.ChainGenerator over the table; flags = GLOBAL_ROWS, no weights: _vote_oracle.Generator's own loop (ssdr_vote_tiles_dev)"""
    return FO.ChainGenerator(table.clouds, poss, N, SCALE, xy_only=bool(flags & XY_ONLY), global_rows=bool(flags & GLOBAL_ROWS), class_weight=weights,
                             activation=table.acts if channels else None, pseudo=table.pses if channels else None)


def next_pick(gen):
    """(cloud, point) the generator's next tile starts from"""
    c = int(np.argmin(np.asarray(gen.min_possibility)))
    return c, int(np.argmin(gen.possibility[c]))


def chain_reference(gen, table, draws, centre=None):
    """gen.batch(draws), tile by tile; centre: every tile's noise is first replaced by the one that puts its centre there (the draws are changed in place).
    -> the batch and the state after it (map, cloud minima, cloud arg-minima)"""
    tiles = []
    for t in range(len(draws["noise"])):
        if centre is not None:
            draws["noise"][t] = towards(table, *next_pick(gen), centre)
        tiles.append(gen.tile(draws["noise"][t], draws["perm"][t], draws["dup"][t]))
    out = {k: np.stack([x[k] for x in tiles]) for k in tiles[0] if k != "cloud"}
    out["cloud"] = np.array([x["cloud"] for x in tiles], np.int32)
    return out, oracle_state(gen)


def oracle_state(gen):
    return np.concatenate(gen.possibility).copy(), np.asarray(gen.min_possibility, np.float64).copy(), gen.cloud_arg()


def indep_reference(table, tile_cloud, tile_point, draws, N):
    out = FO.indep_batch(table.clouds, table.acts, table.pses, tile_cloud, tile_point, draws, N, SCALE)
    out["cloud"] = np.asarray(tile_cloud, np.int32)
    return out


# ---- callers ----------------------------------------------------------------------------------------------------------------------------------------------
class Table:
    """a table on the device, every copy and call ordered on `stream` (None: the library's); with a map: ssdr_vote_init_dev at once"""

    def __init__(self, table, poss=None, stream=None):
        from ssdr_al import _lib
        _lib.check(_lib.lib().ssdr_init(0))
        self.t, self.stream, self.nc = table, stream, len(table.clouds)
        up = self.up
        self.d_p = up(np.concatenate([c["xyz"] for c in table.clouds]))
        self.d_c = up(np.concatenate([c["rgb"] for c in table.clouds]).astype(F32))
        self.d_l = up(np.concatenate([c["labels"] for c in table.clouds]).astype(np.int32))
        self.d_a, self.d_s = up(np.concatenate(table.acts)), up(np.concatenate(table.pses))
        self.d_poss = None
        if poss is not None:
            self.d_poss = up(np.concatenate(poss).astype(np.float64))
            self.d_min, self.d_arg = up(np.full(self.nc, 7.5, np.float64)), up(np.full(self.nc, SENTINEL_I, np.int32))
            self.init()

    def up(self, a):
        from ssdr_al._lib import DevArray
        return DevArray.from_host(a, stream=self.stream)

    def init(self):
        from ssdr_al import _lib
        _lib.check(_lib.lib().ssdr_vote_init_dev(self.d_poss.ptr, _lib.ptr(self.t.off), self.nc, self.d_min.ptr, self.d_arg.ptr, self.stream))

    def set_map(self, poss):
        """another map over the same table: uploaded, then ssdr_vote_init_dev again -> (cloud_min, cloud_arg)"""
        self.d_poss = self.up(np.concatenate(poss).astype(np.float64))
        self.d_min, self.d_arg = self.up(np.full(self.nc, 7.5, np.float64)), self.up(np.full(self.nc, SENTINEL_I, np.int32))
        self.init()
        return self.state()[1:]

    def state(self):
        """(map, cloud_min, cloud_arg)"""
        return tuple(d.to_host(stream=self.stream) for d in (self.d_poss, self.d_min, self.d_arg))

    def _outputs(self, B, N, feat, labels, channels, cdim):
        o = dict(xyz=np.full((B, N, 3), SENTINEL_F, F32), idx=np.full((B, N), SENTINEL_I, np.int32), cloud=np.full((B,), SENTINEL_I, np.int32),
                 center=np.full((B, 3), SENTINEL_F, F32))
        if feat:
            o["feat"] = np.full((B, N, 3 + cdim), SENTINEL_F, F32)
        if labels:
            o["labels"] = np.full((B, N), SENTINEL_I, np.int32)
        if channels:
            o["act"], o["pse"] = np.full((B, N), SENTINEL_F, F32), np.full((B, N), SENTINEL_F, F32)
        return {k: self.up(v) for k, v in o.items()}

    def _draws(self, draws, B, N):
        assert draws["noise"].shape == (B, 3) and draws["perm"].shape == (B, N) and draws["dup"].shape == (B, N)
        return self.up(draws["noise"]), self.up(draws["perm"]), self.up(draws["dup"])

    def _down(self, o):
        from ssdr_al import _lib
        _lib.sync(self.stream)
        return {k: v.to_host(stream=self.stream) for k, v in o.items()}

    def chain(self, draws, N, flags=GLOBAL_ROWS, weights=None, channels=True, feat=True, labels=True, colors=True, entry="feed"):
        """ssdr_feed_chain_dev (entry "vote": ssdr_vote_tiles_dev, which has neither flags, weights nor channels); feat / labels / channels False: those outputs
        NULL; colors False: the colours NULL and color_dim 0.  Outputs prefilled with a sentinel.  -> every present output, host arrays"""
        from ssdr_al import _lib
        L = _lib.lib()
        B = len(draws["noise"])
        cdim = 3 if colors else 0
        d_n, d_perm, d_dup = self._draws(draws, B, N)
        channels = channels and entry != "vote"
        o = self._outputs(B, N, feat, labels, channels, cdim)
        g = lambda k: o[k].ptr if k in o else None
        head = (self.d_p.ptr, self.d_c.ptr if colors else None, cdim, self.d_l.ptr, self.d_poss.ptr, self.d_min.ptr, self.d_arg.ptr, _lib.ptr(self.t.off), self.nc, B, N,
                d_n.ptr, d_perm.ptr, d_dup.ptr, float(SCALE), g("xyz"), g("feat"), g("idx"), g("labels"), g("cloud"), g("center"))
        if entry == "vote":
            assert flags == GLOBAL_ROWS and weights is None
            _lib.check(L.ssdr_vote_tiles_dev(*head, self.stream))
        else:
            d_w = None if weights is None else self.up(np.ascontiguousarray(weights, np.float64))
            _lib.check(L.ssdr_feed_chain_dev(*head, flags, d_w.ptr if d_w else None, 0 if weights is None else len(weights), self.d_a.ptr if channels else None,
                                             self.d_s.ptr if channels else None, g("act"), g("pse"), self.stream))
        return self._down(o)

    def tiles(self, tile_cloud, tile_point, draws, N):
        """ssdr_feed_tiles_dev -> every output"""
        from ssdr_al import _lib
        B = len(tile_cloud)
        d_n, d_perm, d_dup = self._draws(draws, B, N)
        d_tc, d_tp = self.up(np.asarray(tile_cloud, np.int32)), self.up(np.asarray(tile_point, np.int32))
        o = self._outputs(B, N, True, True, True, 3)
        _lib.check(_lib.lib().ssdr_feed_tiles_dev(self.d_p.ptr, self.d_c.ptr, 3, self.d_l.ptr, self.d_a.ptr, self.d_s.ptr, _lib.ptr(self.t.off), self.nc, B, N, d_tc.ptr, d_tp.ptr,
                                                  d_n.ptr, d_perm.ptr, d_dup.ptr, float(SCALE), o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr, o["labels"].ptr, o["act"].ptr,
                                                  o["pse"].ptr, o["cloud"].ptr, o["center"].ptr, self.stream))
        return self._down(o)


def feed_status(stream=None):
    """ssdr_feed_status -> (return code, status bits); reading clears the bits"""
    from ssdr_al import _lib
    st = np.full(1, SENTINEL_I, np.int32)
    rc = _lib.lib().ssdr_feed_status(stream, _lib.ptr(st))
    return rc, int(st[0])


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("cloud", "center", "idx", "xyz", "feat", "labels", "act", "pse")


def compare(got, ref, what, tiles=None):
    """every output the call produced against the oracle's, bit for bit; tiles: only those (a call with refused tiles among good ones)"""
    sel = slice(None) if tiles is None else np.asarray(tiles)
    for k in OUTPUTS:
        if k not in got:
            continue
        g, r = got[k][sel], ref[k][sel]
        if k == "feat":
            r = r[..., :g.shape[-1]]
        assert g.dtype == r.dtype, "%s %s: %s against %s" % (what, k, g.dtype, r.dtype)
        assert_bits_equal(g, r, "%s %s" % (what, k))


def compare_state(dev, state, what):
    """the float64 map, cloud_min and cloud_arg against the oracle's, bit for bit"""
    got = dev.state()
    assert_bits_equal(got[0].view(np.uint64), state[0].view(np.uint64), what + " map")
    assert_bits_equal(got[1].view(np.uint64), state[1].view(np.uint64), what + " cloud_min")
    assert np.array_equal(got[2], state[2]), "%s cloud_arg: %s, oracle %s" % (what, got[2][got[2] != state[2]][:4], state[2][got[2] != state[2]][:4])


def zero_tile(got, t, what):
    """a refused tile: zeros in every output"""
    for k, v in got.items():
        assert not v[t].any(), "%s: tile %d %s is not zero" % (what, t, k)
