"""Whole-cloud inference over ragged batches: the network pass of the reference's active-learning round.

TSampler.prediction() (S3/sampler2.py:580-642) and compute_features() (:313-342) put every sub-sampled room through the network WHOLE:
spatially_regular_gen in mode "sampling" (s3dis_dataset.py:115-154) queries all its points around a noisy pick point, shuffles them, pads a
room smaller than num_points by duplication, builds the KNN pyramid over the whole cloud (tf_map, :156-183), and the outputs are read back
in the room's own point order (prob_logits[np.argsort(point_idx[0])], sampler2.py:599; last_second_features likewise, :327).

WholeCloudPredictor runs a list of such clouds as chunks of at most `max_rows` level-0 rows.  Per chunk, on one stream: the whole-cloud
tile (ssdr_predict_tile_dev), the KNN pyramid of every cloud (ssdr_knn_pyramid_ragged_dev), the translation of its tables into the packed
row space (ssdr_predict_translate_dev), ONE B = 1 network call over the packed rows (ssdr_randla_infer_rows_dev) and the read-back into each
cloud's point order (ssdr_predict_readback_dev).  The packing is described in csrc/predict.hip and include/ssdr_al.h.

dataset="Semantic3D": the flavour of Semantic3D_Dataset_Sampling in mode "sampling" (SSRD_AL_semantic3d/semantic3d_dataset_sampling.py:114-294) with
TSampler.prediction() / compute_features() (sampler2.py:320-360, :598-670): a scan is never padded, its features are augmented, split3 and the
merge rule cut it into parts, every part has a pyramid and network rows of its own, and the outputs go back with total[point_idx[0]] = out
(DESIGN.md section 27)."""
import ctypes as C

import numpy as np

from . import _lib, randlanet
from . import draws as device_draws
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
    carry none), offsets host int64 [n_clouds + 1] — the arrays HotPath.from_device takes.  The Semantic3D flavour adds part_offsets / parts
    (how split3 cut every scan) and keeps the tiles (t_xyz, t_feat, t_idx) and the split's order in `inputs`."""

    def __init__(self, probs, feat32, inputs, offsets, stream, chunks):
        self.probs, self.feat32, self.offsets = probs, feat32, offsets
        self.xyz, self.labels = inputs["xyz"], inputs["labels"]
        self.stream = stream
        # every buffer the enqueued work reads or writes stays referenced as long as the result: DevArray's pool hands a dropped
        # buffer to the next allocation at once, whatever stream that allocation is used on
        self.inputs = inputs
        self.chunks = chunks          # per chunk (input order): its layout and device buffers
        self.part_offsets = None      # the Semantic3D flavour: per scan int64 [parts + 1], ranges of its stretch of inputs["order"]

    @property
    def parts(self):
        """The Semantic3D flavour: per scan dict(offsets int64 [parts + 1], rows = the tile rows of each part, int32, in the order the network
        saw them).  Host copies: waits for the stream.  None for the S3DIS flavour."""
        if self.part_offsets is None:
            return None
        order = self.inputs["order"].to_host(self.stream)
        o = self.offsets
        return [dict(offsets=off, rows=[order[o[c] + off[k]:o[c] + off[k + 1]] for k in range(len(off) - 1)]) for c, off in enumerate(self.part_offsets)]

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


class _Slice(DevArray):
    """`shape` elements of a DevArray from element `first` on: no buffer of its own"""

    def __init__(self, base, first, shape):
        self.shape, self.dtype, self._base = tuple(int(x) for x in shape), base.dtype, base
        self.ptr = base.ptr + int(first) * base.dtype.itemsize
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        assert int(first) * base.dtype.itemsize + self.nbytes <= base.nbytes

    def __del__(self):
        pass


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

    def __init__(self, weights, config=ConfigS3DIS, precision="f32", tiles32=True, max_rows=1 << 22, dataset="S3DIS", split_max=800000,
                 split_recurse_max=800000, merge_max=2000, color_scale=1.0, draws="host", keep_chunks=True):
        """dataset="Semantic3D" (see run): split_max / split_recurse_max / merge_max are split3's top-level bound, the bound its recursive calls
        use (the reference passes the literal 800000 there) and the merge rule's; color_scale multiplies the colours (the S3DIS flavour keeps its
        1 / 255); draws="device" makes the per-row draws (shuffle, augmentation noise) on the stream; keep_chunks=False lets a chunk's device
        buffers go back to the pool once its read-back is enqueued (stream order makes the reuse safe) and keeps the chunks' layouts alone."""
        if dataset not in ("S3DIS", "Semantic3D"):
            raise ValueError("WholeCloudPredictor: dataset must be 'S3DIS' or 'Semantic3D'")
        if draws not in ("host", "device"):
            raise ValueError("WholeCloudPredictor: draws must be 'host' or 'device'")
        if max_rows > MAX_ROWS:
            raise _lib.SsdrError(SSDR_ERR_UNSUPPORTED, "WholeCloudPredictor: max_rows %d above the cap of %d (2^23) level-0 rows" % (max_rows, MAX_ROWS))
        if dataset == "S3DIS" and max_rows < config.num_points:
            raise ValueError("max_rows %d below one tile of %d rows" % (max_rows, config.num_points))
        if max_rows < 1:
            raise ValueError("max_rows %d below one row" % max_rows)
        self.dataset, self.draws, self.keep_chunks = dataset, draws, bool(keep_chunks)
        self.split_max, self.split_recurse_max, self.merge_max = int(split_max), int(split_recurse_max), int(merge_max)
        self.color_scale = float(color_scale)
        self.augment_noise = float(getattr(config, "augment_noise", 0.0))
        self.poison = None          # tests: a value the outputs are filled with before the Semantic3D pass is enqueued
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
        if self.dataset == "Semantic3D":
            if readback != "reference":
                raise ValueError("WholeCloudPredictor: the Semantic3D pass holds every point once: readback=%r is refused (leave the default)" % (readback,))
            return self._run_scans(clouds, seed, room_ids, stream, draws)
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

    # ---- the Semantic3D flavour ---------------------------------------------------------------------------------------------------------
    def draw_scan(self, xyz, rid, seed):
        """The draws of one whole scan, a function of (seed, room id): the noisy pick point (semantic3d_dataset_sampling.py:119-127), then rot =
        (cos, sin) of theta = uniform(0, 2 pi), scale [3] = uniform(scale_min, scale_max) times the symmetry signs (as TrainFeeder.draw builds
        its Semantic3D entries, from cfg.augment_*), then per row the shuffle perm int32 [n] (:137) and aug_noise float64 [n,3] = normal(0,
        augment_noise) (None when that is 0).  draws="device": without the two per-row entries."""
        cfg = self.cfg
        rng = np.random.default_rng([seed, rid])
        n = len(xyz)
        pick = xyz[rng.integers(0, n)] + rng.normal(0, cfg.noise_init / 10, 3)
        theta = rng.uniform(0, 2 * np.pi, size=1)
        lo, hi = getattr(cfg, "augment_scale_min", 1.0), getattr(cfg, "augment_scale_max", 1.0)
        s = rng.uniform(lo, hi, size=(1, 3)) if getattr(cfg, "augment_scale_anisotropic", True) else np.repeat(rng.uniform(lo, hi, size=(1, 1)), 3, axis=1)
        sym = np.ones((1, 3))
        for i, on in enumerate(getattr(cfg, "augment_symmetries", [False, False, False])):
            if on:
                sym[:, i] = np.round(rng.uniform(size=1)) * 2 - 1
        d = dict(center=np.ascontiguousarray(pick, np.float32), rot=np.array([np.cos(theta[0]), np.sin(theta[0])]), scale=(s * sym)[0])
        if self.draws == "host":
            d.update(perm=rng.permutation(n).astype(np.int32),
                     aug_noise=rng.normal(scale=self.augment_noise, size=(n, 3)) if self.augment_noise != 0 else None)
        return d

    @staticmethod
    def device_seed(seed, rid):
        """the 64-bit seed of a scan's device draws: counter (this seed, epoch 0, step 0, kind, element) of ssdr_al.draws"""
        return int(np.random.SeedSequence([int(seed), int(rid), 1]).generate_state(1, np.uint64)[0])

    def part_chunks(self, rows):
        """parts (their level-0 rows, in order) grouped into chunks of at most max_rows rows and 4096 parts (a larger part runs alone)"""
        out, lo, acc = [], 0, 0
        for i, n in enumerate(rows):
            if i > lo and (acc + int(n) > self.max_rows or i - lo >= 4096):
                out.append((lo, i)); lo, acc = i, 0
            acc += int(n)
        if len(rows):
            out.append((lo, len(rows)))
        return out

    def _run_scans(self, clouds, seed, room_ids, stream, draws):
        """The Semantic3D pass.  Per scan, on `stream`: the unpadded tile (ssdr_predict_scan_tile_dev), tf_augment_input over the whole tile
        (ssdr_feed_augment_dev), split3 + merge on the centred, shuffled coordinates (ssdr_split3_dev).  The split is SYNCHRONOUS: the host
        decides its recursion tree, so run() waits for the stream once per scan (more often when a part is split again).  Then the parts of
        all scans, in order, in chunks: ssdr_predict_parts_dev, the ragged pyramid, the translation, one network call and
        ssdr_predict_scatter_dev per chunk, enqueued without a further wait.  Nothing between the tile and the read-back goes through the
        host but the split's tree."""
        cfg, Lib = self.cfg, _lib.lib()
        L, K, Cn = cfg.num_layers, cfg.k_n, cfg.num_classes
        sizes = [len(c["xyz"]) for c in clouds]
        for i, n in enumerate(sizes):
            if n == 0:
                raise _lib.SsdrError(1, "WholeCloudPredictor: scan %d is empty (every scan needs at least one point)" % i)
        if room_ids is None:
            room_ids = list(range(len(clouds)))
        if draws is None:
            draws = [self.draw_scan(np.asarray(c["xyz"], np.float32), rid, seed) for c, rid in zip(clouds, room_ids)]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        npts = int(offsets[-1])
        if npts >= 1 << 30:
            raise _lib.SsdrError(SSDR_ERR_UNSUPPORTED, "WholeCloudPredictor: %d points in one run (below 2^30: int32 sources)" % npts)
        noisy = self.augment_noise != 0 or any(d.get("aug_noise") is not None for d in draws)
        for i, (d, n) in enumerate(zip(draws, sizes)):
            if d.get("perm") is not None and (len(d["perm"]) != n or not np.array_equal(np.sort(np.asarray(d["perm"])), np.arange(n))):
                raise ValueError("draws: scan %d: perm must be a permutation of its %d rows" % (i, n))
            if d.get("aug_noise") is not None and np.shape(d["aug_noise"]) != (n, 3):
                raise ValueError("draws: scan %d: aug_noise must be [%d, 3]" % (i, n))
            if self.draws == "host" and (d.get("perm") is None or (noisy and d.get("aug_noise") is None)):
                raise ValueError("draws: scan %d: perm%s missing (draws='host')" % (i, " / aug_noise" if noisy else ""))
        has_lab = all(c.get("labels") is not None for c in clouds)
        cat = lambda key, dt: np.concatenate([np.asarray(c[key], dt).reshape(len(c["xyz"]), -1) for c in clouds])
        inputs = dict(xyz=DevArray.from_host(cat("xyz", np.float32), stream), rgb=DevArray.from_host(cat("rgb", np.float32), stream),
                      labels=DevArray.from_host(cat("labels", np.int32).reshape(-1), stream) if has_lab else None,
                      rot=DevArray.from_host(np.stack([np.asarray(d["rot"], np.float64) for d in draws]), stream),
                      scale=DevArray.from_host(np.stack([np.asarray(d["scale"], np.float64) for d in draws]), stream))
        # the per-row draws: one upload when every scan brings its own, otherwise scan by scan (a key the dict holds is uploaded, the rest
        # is drawn on the stream)
        host_rows = lambda key: all(d.get(key) is not None for d in draws)
        perm = inputs["perm"] = (DevArray.from_host(np.concatenate([np.asarray(d["perm"], np.int32) for d in draws]), stream) if host_rows("perm")
                                 else DevArray((npts,), np.int32))
        noise = None
        if noisy:
            noise = (DevArray.from_host(np.concatenate([np.asarray(d["aug_noise"], np.float64) for d in draws]), stream) if host_rows("aug_noise")
                     else DevArray((npts, 3), np.float64))
        inputs["aug_noise"] = noise
        for c, (d, rid) in enumerate(zip(draws, room_ids)):
            o, n = int(offsets[c]), sizes[c]
            ds = self.device_seed(seed, rid)
            if not host_rows("perm"):
                if d.get("perm") is not None:
                    a = np.ascontiguousarray(d["perm"], np.int32)
                    _lib.check(Lib.ssdr_memcpy_h2d_on(perm.ptr + 4 * o, _lib.ptr(a), a.nbytes, stream))
                else:
                    device_draws.perm(ds, 0, 0, 1, n, out=_Slice(perm, o, (1, n)), stream=stream)
            if noisy and not host_rows("aug_noise"):
                if d.get("aug_noise") is not None:
                    a = np.ascontiguousarray(d["aug_noise"], np.float64)
                    _lib.check(Lib.ssdr_memcpy_h2d_on(noise.ptr + 24 * o, _lib.ptr(a), a.nbytes, stream))
                else:
                    device_draws.normal(ds, 0, 0, device_draws.AUG_NOISE, 3 * n, scale=self.augment_noise, out=_Slice(noise, 3 * o, (3 * n,)), stream=stream)
        probs = DevArray((npts, Cn), np.float32)
        feat = DevArray((npts, 32), np.float32)
        if self.poison is not None:
            for a in (probs, feat):
                h = np.full(a.shape, self.poison, np.float32)
                _lib.check(Lib.ssdr_memcpy_h2d_on(a.ptr, _lib.ptr(h), h.nbytes, stream))
        t_xyz = inputs["t_xyz"] = DevArray((npts, 3), np.float32)
        t_feat = inputs["t_feat"] = DevArray((npts, 6), np.float32)
        t_idx = inputs["t_idx"] = DevArray((npts,), np.int32)
        order = inputs["order"] = DevArray((npts,), np.int32)
        # tile, features, split: scan by scan
        cap = 4096
        part_off, part_scan, scan_parts = [0], [], []
        for c, d in enumerate(draws):
            o, n = int(offsets[c]), sizes[c]
            center = np.ascontiguousarray(d["center"], np.float32)
            _lib.check(Lib.ssdr_predict_scan_tile_dev(inputs["xyz"].ptr + 12 * o, inputs["rgb"].ptr + 12 * o, n, _lib.ptr(center), perm.ptr + 4 * o,
                                                      self.color_scale, t_xyz.ptr + 12 * o, t_feat.ptr + 24 * o, t_idx.ptr + 4 * o, stream))
            _lib.check(Lib.ssdr_feed_augment_dev(t_xyz.ptr + 12 * o, 1, n, inputs["rot"].ptr + 16 * c, inputs["scale"].ptr + 24 * c,
                                                 noise.ptr + 24 * o if noise is not None else None, 3, t_feat.ptr + 24 * o, stream))
            off = np.zeros(cap + 1, np.int64); num = C.c_size_t()
            _lib.check(Lib.ssdr_split3_dev(t_xyz.ptr + 12 * o, n, self.split_max, self.split_recurse_max, self.merge_max, None, order.ptr + 4 * o,
                                           _lib.ptr(off), cap, C.byref(num), stream))
            off = off[: num.value + 1].copy()
            for k in range(num.value):
                rows = int(off[k + 1] - off[k])
                if level_sizes(rows, self.ratios)[-1] <= 0:
                    raise _lib.SsdrError(1, "WholeCloudPredictor: scan %d, part %d (%d rows) is too small for the pyramid" % (c, k, rows))
                part_off.append(o + int(off[k + 1])); part_scan.append(c)
            scan_parts.append(off)
        part_off = np.asarray(part_off, np.int64)
        part_base = offsets[np.asarray(part_scan, np.int64)].astype(np.int64)
        chunks = []
        for lo, hi in self.part_chunks(np.diff(part_off)):
            b = self._enqueue_parts(lo, hi, part_off, part_base, part_scan, scan_parts, inputs, probs, feat, npts, has_lab, stream)
            chunks.append(b if self.keep_chunks else {k: v for k, v in b.items() if not isinstance(v, DevArray)})
        out = Prediction(probs, feat, inputs, offsets, stream, chunks)
        out.part_offsets = scan_parts          # per scan: int64 [its parts + 1], ranges of its stretch of the split's order
        return out

    def _enqueue_parts(self, lo, hi, part_off, part_base, part_scan, scan_parts, inputs, probs, feat, npts, has_lab, stream):
        """one chunk of parts: allocation and launch sequence on `stream` (no host wait)"""
        cfg, Lib = self.cfg, _lib.lib()
        L, K, Cn = cfg.num_layers, cfg.k_n, cfg.num_classes
        np_ = hi - lo
        abs_off = np.ascontiguousarray(part_off[lo:hi + 1])
        base = np.ascontiguousarray(part_base[lo:hi])
        off = (abs_off - abs_off[0]).astype(np.int64)
        T = [int(x) for x in np.diff(off)]
        r, o = _lib.ptr(self.ratios), _lib.ptr(off)
        P = np.zeros(L + 1, np.int64)
        _lib.check(Lib.ssdr_predict_layout(o, np_, 1, L, r, _lib.ptr(P)))
        R = np.concatenate([[0], np.cumsum(P[:L])]).astype(np.int64)
        rows, kr = int(sum(T)), int(R[L])
        first = {}
        for c in part_scan[lo:hi]:
            first.setdefault(c, part_scan.index(c))
        b = dict(T=T, P=P, R=R, off=off, lo=lo, hi=hi, p0=int(abs_off[0]), r0=int(abs_off[0]), centers=None, cm_idx=None,
                 parts=[(c, lo + k - first[c]) for k, c in enumerate(part_scan[lo:hi])], part_base=base, part_off=abs_off)
        b["cm_xyz"] = DevArray((rows, 3), np.float32)
        b["pk_xyz"] = DevArray((rows, 3), np.float32); b["pk_feat"] = DevArray((rows, 6), np.float32)
        b["pk_src"] = DevArray((rows,), np.int32)
        b["pk_lab"] = DevArray((rows,), np.int32) if has_lab else None
        b["cm_neigh"] = DevArray((kr, K), np.int32); b["cm_interp"] = DevArray((kr,), np.int32)
        b["pk_neigh"] = DevArray((kr, K), np.int32); b["pk_interp"] = DevArray((kr,), np.int32)
        b["pk_probs"] = DevArray((rows, Cn), np.float32); b["pk_f32"] = DevArray((rows, 32), np.float32)
        labels = inputs["labels"]
        _lib.check(Lib.ssdr_predict_parts_dev(inputs["t_xyz"].ptr, inputs["t_feat"].ptr, inputs["t_idx"].ptr, labels.ptr if has_lab else None,
                                              inputs["order"].ptr, _lib.ptr(abs_off), _lib.ptr(base), np_, L, r, b["cm_xyz"].ptr, b["pk_xyz"].ptr,
                                              b["pk_feat"].ptr, b["pk_src"].ptr, b["pk_lab"].ptr if has_lab else None, stream))
        _lib.check(Lib.ssdr_knn_pyramid_ragged_dev(b["cm_xyz"].ptr, o, np_, 1, L, r, K, b["cm_neigh"].ptr, b["cm_interp"].ptr, stream))
        _lib.check(Lib.ssdr_predict_translate_dev(o, np_, 1, L, r, K, b["cm_neigh"].ptr, b["cm_interp"].ptr, b["pk_neigh"].ptr, b["pk_interp"].ptr, stream))
        arr = C.c_void_p * L
        lv = (C.c_size_t * (L + 1))(*[int(x) for x in P])
        _lib.check(Lib.ssdr_randla_infer_rows_dev(self.net._h, lv, b["pk_feat"].ptr, b["pk_xyz"].ptr,
                                                  arr(*[b["pk_neigh"].ptr + 4 * K * int(R[l]) for l in range(L)]),
                                                  arr(*[b["pk_interp"].ptr + 4 * int(R[l]) for l in range(L)]),
                                                  b["pk_probs"].ptr, b["pk_f32"].ptr, stream))
        _lib.check(Lib.ssdr_predict_scatter_dev(b["pk_src"].ptr, rows, b["pk_probs"].ptr, Cn, b["pk_f32"].ptr, npts, probs.ptr, feat.ptr, stream))
        return b
