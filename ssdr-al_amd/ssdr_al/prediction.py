"""Whole-cloud inference over ragged batches: the network pass of the reference's active-learning round.

TSampler.prediction() (S3/sampler2.py:580-642) and compute_features() (:313-342) put every sub-sampled room through the network WHOLE:
spatially_regular_gen in mode "sampling" (s3dis_dataset.py:115-154) queries all its points around a noisy pick point, shuffles them, pads a
room smaller than num_points by duplication, builds the KNN pyramid over the whole cloud (tf_map, :156-183), and the outputs are read back
in the room's own point order (prob_logits[np.argsort(point_idx[0])], sampler2.py:599; last_second_features likewise, :327).

WholeCloudPredictor runs a list of such clouds as chunks of at most `max_rows` level-0 rows.  Per chunk, on one stream: the whole-cloud
tile (ssdr_predict_tile_dev), the KNN pyramid of every cloud (ssdr_knn_pyramid_ragged_dev), the translation of its tables into the packed
row space (ssdr_predict_translate_dev), ONE B = 1 network call over the packed rows (ssdr_randla_infer_rows_dev) and the read-back into each
cloud's point order (ssdr_predict_readback_dev).  The packing is described in csrc/predict.hip and include/ssdr_al.h."""
import ctypes as C

import numpy as np

from . import _lib, randlanet
from ._lib import DevArray
from .helper_tool import ConfigS3DIS

MAX_ROWS = 1 << 23          # SSDR_PREDICT_MAX_ROWS: the network's int32 element offsets at that many level-0 rows
READBACK = {"reference": 0, "point": 1}
SSDR_ERR_UNSUPPORTED = 5


def level_sizes(T, ratios):
    """N^(0) = T, N^(l+1) = N^(l) // ratio[l] (tf_map)"""
    out = [int(T)]
    for r in ratios:
        out.append(out[-1] // int(r))
    return out


def packed_positions(T_list, ratios):
    """NumPy statement of the packing: for every cloud c the packed row of each of its tile rows (int64 [T_c]).  Segment s = L .. 0 holds
    rows [N_c^(s+1), N_c^(s)) of every cloud in turn; the level-l rows of all clouds are then the first P_l packed rows."""
    L = len(ratios)
    lim = [level_sizes(T, ratios) + [0] for T in T_list]
    pos = [np.empty(T, np.int64) for T in T_list]
    at = 0
    for s in range(L, -1, -1):
        for c, lc in enumerate(lim):
            k = lc[s] - lc[s + 1]
            pos[c][lc[s + 1]:lc[s]] = np.arange(at, at + k)
            at += k
    return pos


class Prediction:
    """What WholeCloudPredictor.run returns: device arrays concatenated by cloud, each cloud in its own point order.
    probs [sum n_c, C], feat32 [sum n_c, 32], xyz [sum n_c, 3] and labels [sum n_c] (inputs passed through; labels None when the clouds
    carry none), offsets host int64 [n_clouds + 1] — the arrays HotPath.from_device takes."""

    def __init__(self, probs, feat32, inputs, offsets, stream, chunks):
        self.probs, self.feat32, self.offsets = probs, feat32, offsets
        self.xyz, self.labels = inputs["xyz"], inputs["labels"]
        self.stream = stream
        # every buffer the enqueued work reads or writes stays referenced as long as the result: DevArray's pool hands a dropped
        # buffer to the next allocation at once, whatever stream that allocation is used on
        self.inputs = inputs
        self.chunks = chunks          # per chunk (input order): its layout and device buffers

    def check(self):
        """Waits for the stream and raises SsdrError if a KNN call of this run (or earlier on the stream) left a device status bit set
        (capacity overflows of the grid / tree hand-over: the neighbour lists would not be trustworthy)."""
        st = (C.c_int32 * 4)()
        _lib.check(_lib.lib().ssdr_knn_status(self.stream, st))
        return list(st)

    def to_host(self):
        """Synchronises; one dict per cloud: probs [n,C], feat32 [n,32], xyz [n,3], labels [n] (or None)."""
        _lib.sync(self.stream)
        p, f, x = self.probs.to_host(self.stream), self.feat32.to_host(self.stream), self.xyz.to_host(self.stream)
        lab = self.labels.to_host(self.stream) if self.labels is not None else None
        o = self.offsets
        return [dict(probs=p[o[c]:o[c + 1]], feat32=f[o[c]:o[c + 1]], xyz=x[o[c]:o[c + 1]],
                     labels=None if lab is None else lab[o[c]:o[c + 1]]) for c in range(len(o) - 1)]


class WholeCloudPredictor:
    """The AL round's prediction pass over clouds of any size:

        pred = WholeCloudPredictor(weights, config=ConfigS3DIS, precision="f32", tiles32=True, max_rows=1 << 22)
        out = pred.run(clouds, seed=0, room_ids=None, readback="reference", stream=None)

    ONE pass gives both outputs.  The reference runs two separate network passes with separate random draws: prediction() for the
    probabilities, compute_features() for last_second_features.  Here both come from the same tile (as ALRound does); a caller who wants
    the reference's two draws calls run() twice with two seeds.

    readback: "reference" reproduces out[p] = tile_out[argsort(point_idx)[p]] with a STABLE argsort (on a padded room point_idx holds
    duplicates, so row p is the p-th smallest key's row, not always point p's; NumPy's default argsort is not stable and may pick another
    row of the same point, which differs only in rounding); "point" gives every point the output of its own first tile row.  Identical
    for unpadded clouds."""

    def __init__(self, weights, config=ConfigS3DIS, precision="f32", tiles32=True, max_rows=1 << 22):
        if max_rows > MAX_ROWS:
            raise _lib.SsdrError(SSDR_ERR_UNSUPPORTED, "WholeCloudPredictor: max_rows %d above the cap of %d (2^23) level-0 rows" % (max_rows, MAX_ROWS))
        if max_rows < config.num_points:
            raise ValueError("max_rows %d below one tile of %d rows" % (max_rows, config.num_points))
        self.cfg = config
        self.max_rows = int(max_rows)
        self.net = randlanet.Network(config).load(weights).set_precision(precision).set_formulation(tiles32)
        self.ratios = np.asarray(config.sub_sampling_ratio, np.int32)

    def draw(self, xyz, rid, seed):
        """The host-drawn randomness of one whole cloud, a function of (seed, room id) as HotPath.draw_room: the noisy pick point
        (s3dis_dataset.py:119-126), the shuffle of its T = max(n, num_points) rows (:137) and the padding draws (DP.data_aug)."""
        cfg = self.cfg
        rng = np.random.default_rng([seed, rid])
        n = len(xyz)
        T = max(n, cfg.num_points)
        pick = xyz[rng.integers(0, n)] + rng.normal(0, cfg.noise_init / 10, 3)
        return dict(center=np.ascontiguousarray(pick, np.float32), perm=rng.permutation(T).astype(np.int32), dup=rng.random(T).astype(np.float32))

    def chunks(self, sizes):
        """clouds grouped in input order into chunks of at most max_rows level-0 rows (a larger cloud runs alone): [(first, end), ...]"""
        out, lo, rows = [], 0, 0
        for i, n in enumerate(sizes):
            T = max(int(n), self.cfg.num_points)
            if i > lo and (rows + T > self.max_rows or i - lo >= 4096):
                out.append((lo, i)); lo, rows = i, 0
            rows += T
        if len(sizes):
            out.append((lo, len(sizes)))
        return out

    def layout(self, sizes):
        """P_0 .. P_L of one chunk (validates it: an empty cloud, too many rows)"""
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        P = np.zeros(self.cfg.num_layers + 1, np.int64)
        _lib.check(_lib.lib().ssdr_predict_layout(_lib.ptr(off), len(sizes), self.cfg.num_points, self.cfg.num_layers, _lib.ptr(self.ratios), _lib.ptr(P)))
        return P

    def run(self, clouds, seed=0, room_ids=None, readback="reference", stream=None, draws=None):
        """clouds: list of dict(xyz f32 [n,3], rgb [n,3] 0..255, labels int [n] (optional)).  draws (optional): one dict(center, perm, dup)
        per cloud instead of draw() (tests hand the same draws to a NumPy restatement).

        Waits: run() first uploads every input (points, colours, labels, every chunk's shuffle and padding draws) and allocates every
        chunk's buffers; each upload waits for its copy on `stream`.  Then it enqueues all chunks on `stream` and returns without waiting.
        The largest chunk goes first, so the library's grow-only workspaces (which synchronise the device when they grow) reach their
        size there.  The result keeps every buffer the enqueued work reads or writes (inputs and out.chunks) until it goes."""
        if readback not in READBACK:
            raise ValueError("readback must be 'reference' or 'point'")
        cfg = self.cfg
        L, K, Cn = cfg.num_layers, cfg.k_n, cfg.num_classes
        sizes = [len(c["xyz"]) for c in clouds]
        for i, n in enumerate(sizes):
            if n == 0:
                raise _lib.SsdrError(1, "WholeCloudPredictor: cloud %d is empty (every cloud needs at least one point)" % i)
        if room_ids is None:
            room_ids = list(range(len(clouds)))
        if draws is None:
            draws = [self.draw(np.asarray(c["xyz"], np.float32), rid, seed) for c, rid in zip(clouds, room_ids)]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        T_all = [max(int(n), cfg.num_points) for n in sizes]
        row_off = np.concatenate([[0], np.cumsum(T_all)]).astype(np.int64)      # every cloud's draws at its row offset
        npts = int(offsets[-1])
        has_lab = all(c.get("labels") is not None for c in clouds)
        # every upload before the first enqueue
        inputs = dict(xyz=DevArray.from_host(np.concatenate([np.asarray(c["xyz"], np.float32) for c in clouds]), stream),
                      rgb=DevArray.from_host(np.concatenate([np.asarray(c["rgb"], np.float32) for c in clouds]), stream),
                      labels=DevArray.from_host(np.concatenate([np.asarray(c["labels"]).astype(np.int32).reshape(-1) for c in clouds]), stream)
                      if has_lab else None,
                      perm=DevArray.from_host(np.concatenate([np.asarray(d["perm"], np.int32) for d in draws]), stream),
                      dup=DevArray.from_host(np.concatenate([np.asarray(d["dup"], np.float32) for d in draws]), stream))
        for d, T in zip(draws, T_all):
            if len(d["perm"]) != T or len(d["dup"]) != T:
                raise ValueError("draws: perm and dup need max(n, num_points) = %d entries" % T)
        probs = DevArray((npts, Cn), np.float32)
        feat = DevArray((npts, 32), np.float32)
        # every chunk's layout and buffers before the first enqueue
        chunks = []
        for lo, hi in self.chunks(sizes):
            off = (offsets[lo:hi + 1] - offsets[lo]).astype(np.int64)
            T = T_all[lo:hi]
            P = self.layout(np.diff(off))
            R = np.concatenate([[0], np.cumsum(P[:L])]).astype(np.int64)
            rows, kr = int(sum(T)), int(R[L])
            b = dict(T=T, P=P, R=R, off=off, lo=lo, hi=hi, p0=int(offsets[lo]), r0=int(row_off[lo]),
                     centers=np.ascontiguousarray(np.stack([np.asarray(d["center"], np.float32) for d in draws[lo:hi]]), np.float32))
            b["cm_xyz"] = DevArray((rows, 3), np.float32); b["cm_idx"] = DevArray((rows,), np.int32)
            b["pk_xyz"] = DevArray((rows, 3), np.float32); b["pk_feat"] = DevArray((rows, 6), np.float32)
            b["pk_src"] = DevArray((rows,), np.int32)
            b["pk_lab"] = DevArray((rows,), np.int32) if has_lab else None
            b["cm_neigh"] = DevArray((kr, K), np.int32); b["cm_interp"] = DevArray((kr,), np.int32)
            b["pk_neigh"] = DevArray((kr, K), np.int32); b["pk_interp"] = DevArray((kr,), np.int32)
            b["pk_probs"] = DevArray((rows, Cn), np.float32); b["pk_f32"] = DevArray((rows, 32), np.float32)
            chunks.append(b)
        for b in sorted(chunks, key=lambda b: -int(b["P"][0])):
            self._enqueue(b, inputs, probs, feat, READBACK[readback], stream)
        return Prediction(probs, feat, inputs, offsets, stream, chunks)

    def _enqueue(self, b, inputs, probs, feat, mode, stream):
        """one chunk's launch sequence on `stream`: tile, pyramid, translation, network, read-back (no host wait, no allocation)"""
        cfg, Lib = self.cfg, _lib.lib()
        L, K, Cn = cfg.num_layers, cfg.k_n, cfg.num_classes
        nc, p0, r0, R, P = b["hi"] - b["lo"], b["p0"], b["r0"], b["R"], b["P"]
        xyz, rgb, labels = inputs["xyz"], inputs["rgb"], inputs["labels"]
        r, o = _lib.ptr(self.ratios), _lib.ptr(b["off"])
        _lib.check(Lib.ssdr_predict_tile_dev(xyz.ptr + 12 * p0, rgb.ptr + 12 * p0, labels.ptr + 4 * p0 if labels is not None else None, o, nc,
                                             _lib.ptr(b["centers"]), cfg.num_points, L, r, inputs["perm"].ptr + 4 * r0, inputs["dup"].ptr + 4 * r0,
                                             1.0 / 255.0, b["cm_xyz"].ptr, b["cm_idx"].ptr, b["pk_xyz"].ptr, b["pk_feat"].ptr, b["pk_src"].ptr,
                                             b["pk_lab"].ptr if b["pk_lab"] is not None else None, stream))
        _lib.check(Lib.ssdr_knn_pyramid_ragged_dev(b["cm_xyz"].ptr, o, nc, cfg.num_points, L, r, K, b["cm_neigh"].ptr, b["cm_interp"].ptr, stream))
        _lib.check(Lib.ssdr_predict_translate_dev(o, nc, cfg.num_points, L, r, K, b["cm_neigh"].ptr, b["cm_interp"].ptr,
                                                  b["pk_neigh"].ptr, b["pk_interp"].ptr, stream))
        arr = C.c_void_p * L
        lv = (C.c_size_t * (L + 1))(*[int(x) for x in P])
        _lib.check(Lib.ssdr_randla_infer_rows_dev(self.net._h, lv, b["pk_feat"].ptr, b["pk_xyz"].ptr,
                                                  arr(*[b["pk_neigh"].ptr + 4 * K * int(R[l]) for l in range(L)]),
                                                  arr(*[b["pk_interp"].ptr + 4 * int(R[l]) for l in range(L)]),
                                                  b["pk_probs"].ptr, b["pk_f32"].ptr, stream))
        _lib.check(Lib.ssdr_predict_readback_dev(o, nc, cfg.num_points, L, r, b["cm_idx"].ptr, b["pk_probs"].ptr, Cn, b["pk_f32"].ptr, mode,
                                                 probs.ptr + 4 * Cn * p0, feat.ptr + 4 * 32 * p0, stream))
