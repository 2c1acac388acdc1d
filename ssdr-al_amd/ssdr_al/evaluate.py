"""Mirror of the evaluation tail of the reference ("next" row N2): vote smoothing, re-projection, confusion, IoU
(/root/reference/SSDR_AL_s3dis/RandLANet.py:326-334, 353-411; helper_tool.py:237-262; utils/data_prepare_s3dis.py:69), and the
test-time voting loop that composes them with the generator chain (VoteTester: RandLANet.py:290-424, s3dis_dataset_test.py:85-151)."""
import ctypes as C

import numpy as np

from . import _lib
from . import draws as device_draws
from ._lib import DevArray
from .knn import knn


def project_indices(sub_xyz, xyz):
    """proj_idx = np.squeeze(KDTree(sub_xyz).query(xyz, return_distance=False)) (data_prepare_s3dis.py:69-70): nearest
    sub-sampled point of every raw point.  Exact nearest neighbour in float32 arithmetic; where two sub-points are
    equidistant the reference's sklearn tree may pick the other one."""
    return knn(sub_xyz, xyz, 1)[:, 0].astype(np.int32)


class VoteAccumulator:
    """test_probs of one cloud, resident on the device (RandLANet.py:292-334)."""

    def __init__(self, num_points, num_classes, test_smooth=0.95):
        self.C, self.smooth = num_classes, float(test_smooth)
        self.test_probs = DevArray.from_host(np.zeros((num_points, num_classes), np.float32))
        self.owner = DevArray.from_host(np.full(num_points, -1, np.int32))

    def update(self, p_idx, probs):
        """test_probs[p_idx] = smooth * test_probs[p_idx] + (1 - smooth) * probs (:333)."""
        d_i = DevArray.from_host(np.ascontiguousarray(p_idx, np.int32)); d_p = DevArray.from_host(np.ascontiguousarray(probs, np.float32))
        _lib.check(_lib.lib().ssdr_vote_smooth_dev(self.test_probs.ptr, d_i.ptr, d_p.ptr, len(p_idx), self.C, self.smooth, self.owner.ptr, None))
        _lib.sync()

    def probs(self):
        return self.test_probs.to_host()

    def confusion(self, labels, proj_idx=None):
        """(preds, confusion int64 [C,C], IoU float64 [C]) on the sub-cloud, or on the raw cloud through proj_idx (:353-405)."""
        lab = np.ascontiguousarray(labels, np.int32)
        n = len(lab)
        d_l = DevArray.from_host(lab)
        d_proj = None if proj_idx is None else DevArray.from_host(np.ascontiguousarray(proj_idx, np.int32))
        d_pred = DevArray((n,), np.int32); d_conf = DevArray.from_host(np.zeros((self.C, self.C), np.uint64)); d_iou = DevArray((self.C,), np.float64)
        _lib.check(_lib.lib().ssdr_confusion_dev(self.test_probs.ptr, self.C, d_proj.ptr if d_proj else None, d_l.ptr, n, d_pred.ptr, d_conf.ptr, d_iou.ptr, None))
        _lib.sync()
        return d_pred.to_host(), d_conf.to_host().astype(np.int64), d_iou.to_host()


def IoU_from_confusions(confusions):
    """helper_tool.py:237-262 for one [C,C] matrix, computed by the device kernel."""
    c = np.ascontiguousarray(confusions, np.uint64)
    C = c.shape[-1]
    d_conf = DevArray.from_host(c); d_iou = DevArray((C,), np.float64)
    d_dummy = DevArray((1,), np.int32); d_p = DevArray((C,), np.float32)
    _lib.check(_lib.lib().ssdr_confusion_dev(d_p.ptr, C, None, d_dummy.ptr, 0, None, d_conf.ptr, d_iou.ptr, None))
    _lib.sync()
    return d_iou.to_host()


def _iou_host(confusions):
    """helper_tool.py:237-262 on a host matrix of any dtype (the rescaled float32 sub-cloud confusion of RandLANet.py:362-368)."""
    c = np.asarray(confusions)
    tp = np.diagonal(c, axis1=-2, axis2=-1)
    tp_fn = np.sum(c, axis=-1)
    tp_fp = np.sum(c, axis=-2)
    iou = tp / (tp_fp + tp_fn - tp + 1e-6)
    mask = tp_fn < 1e-3
    counts = np.sum(1 - mask, axis=-1, keepdims=True)
    miou = np.sum(iou, axis=-1, keepdims=True) / (counts + 1e-6)
    iou += mask * miou
    return iou


class VoteTester:
    """Network.evaluate_test_s3dis (RandLANet.py:290-424) over the test-time generator (s3dis_dataset_test.py:85-151), device-resident.

    ``clouds[c]`` = dict(xyz [n,3], rgb [n,3], labels [n] or None, proj_idx=None, raw_labels=None): the sub-sampled cloud, and
    optionally the raw cloud's nearest sub-point per raw point with the raw labels (val_proj / val_labels); without them the
    "full cloud" is the sub-cloud itself.  All clouds live concatenated on the device together with the possibility map, the
    per-cloud minima and test_probs.  The host draws the randomness (initial map from (seed, cloud), noise / shuffle / padding
    draws from (seed, epoch, step)), reads the cloud minima once per epoch and the final matrices, nothing else.

    ``draws="device"``: the per-row draws (the shuffle permutations, the padding draws) are made on the device from the counter
    (seed, epoch, step, kind, element) instead (``ssdr_al.draws``); ``draw`` then returns the per-tile noise
    alone and nothing per row is uploaded.  The rule is per key: a per-row entry that a ``draws=`` callable does return is uploaded.

    The generator chain (ssdr_vote_tiles_dev) runs on a stream of its own, DEPTH batches ahead of the network at most (the tile
    and draw buffers exist DEPTH times); the draws are uploaded on a third stream, so the host waits for the generator of DEPTH
    batches ago only, never for the network.  ``ready`` guards the draw buffers against the upload
    stream.  A draw made on the device needs no event of its own: it is enqueued on the generator's stream in front of the chain,
    the stream whose chain was the last reader of those buffers, and the set's next upload waits for ``ready`` as before.

    ``dataset="Semantic3D"``: Network.evaluate_test_semantic3d (SSRD_AL_semantic3d/RandLANet.py:339-485) over Semantic3D_Dataset_Test.get_batch
    (semantic3d_dataset_test3.py:129-259).  The generator is the chain's general form (ssdr_feed_chain_dev, flags SSDR_FEED_XY_ONLY |
    SSDR_FEED_GLOBAL_ROWS, no class weights: queried_pt_weight = 1): x / y centred, z kept, the possibility update over all three axes; the
    features are tf_augment_input's over the batch (ssdr_feed_augment_dev; ``draw`` gains rot, scale and aug_noise, built as TrainFeeder.draw
    builds them, aug_noise on the device with ``draws="device"``); colours times ``color_scale``.  ``test_smooth=None`` is 0.95 for S3DIS and
    0.98 for Semantic3D (:343), ``vote_gap=None`` 1 and 4 (:391): the evaluation runs after the first epoch whose smallest possibility
    exceeds last_min + vote_gap.  ``config.ignored_label_inds`` (one value; :403-411, :450-458): rows with that label are dropped from both
    confusions and from OA's count, the other labels shift down by one (done on the host label arrays, as -1 = skipped by
    ssdr_confusion_dev).  A cloud smaller than num_points is refused."""

    DEPTH = 2

    def __init__(self, weights, clouds, config=None, precision="f32", seed=0, num_votes=100, test_smooth=None, possibility=None, draws="host",
                 dataset="S3DIS", vote_gap=None, color_scale=1.0):
        from . import randlanet
        if draws not in ("host", "device"):
            raise ValueError("VoteTester: draws must be 'host' or 'device'")
        self.draws = draws
        if dataset not in ("S3DIS", "Semantic3D"):
            raise ValueError("VoteTester: dataset must be 'S3DIS' or 'Semantic3D'")
        self.dataset = dataset
        sem = self.sem = dataset == "Semantic3D"
        from .helper_tool import ConfigS3DIS, ConfigSemantic3D
        cfg = self.cfg = (ConfigSemantic3D if sem else ConfigS3DIS) if config is None else config
        L = _lib.lib()
        _lib.check(L.ssdr_init(0))
        self.seed, self.num_votes = int(seed), num_votes
        self.test_smooth = float((0.98 if sem else 0.95) if test_smooth is None else test_smooth)
        self.vote_gap = (4 if sem else 1) if vote_gap is None else vote_gap
        self.color_scale = float(color_scale)
        self.augment_noise = float(getattr(cfg, "augment_noise", 0.0)) if sem else 0.0
        self.N, self.B, self.steps, self.C = int(cfg.num_points), int(cfg.val_batch_size), int(getattr(cfg, "val_steps", 100)), int(cfg.num_classes)
        self.nc = len(clouds)
        sizes = [len(c["xyz"]) for c in clouds]
        if sem and sizes and min(sizes) < self.N:
            raise ValueError("VoteTester: a Semantic3D cloud of %d points is smaller than num_points = %d (the reference's tree query raises there)"
                             % (min(sizes), self.N))
        ignored = list(getattr(cfg, "ignored_label_inds", []) or []) if sem else []
        if len(ignored) > 1:
            raise ValueError("VoteTester: ignored_label_inds holds %d values (the reference's labels == ignored_label_inds compares against one)" % len(ignored))
        # :408-410: rows with the ignored label are dropped (-1: ssdr_confusion_dev skips them), the others shift down by one
        relabel = (lambda a: np.where(np.asarray(a) == ignored[0], -1, np.asarray(a) - 1)) if ignored else (lambda a: a)
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n = int(self.off[-1])
        self.has_labels = self.nc > 0 and all(c.get("labels") is not None for c in clouds)
        if possibility is None:
            possibility = [np.random.default_rng([self.seed, c]).random(n) * 1e-3 for c, n in enumerate(sizes)]      # init_possibility, test.py:85-92
        poss = np.concatenate([np.asarray(p, np.float64) for p in possibility]) if self.nc else np.zeros(0)
        cat = lambda key, dt, w: (np.concatenate([np.asarray(c[key], dt).reshape(len(c["xyz"]), *w) for c in clouds]) if self.nc else np.zeros((0, *w), dt))
        self.d_points = DevArray.from_host(cat("xyz", np.float32, (3,)))
        self.d_colors = DevArray.from_host(cat("rgb", np.float32, (3,)))
        self.d_labels = DevArray.from_host(np.ascontiguousarray(relabel(cat("labels", np.int32, ())), np.int32)) if self.has_labels else None
        self.d_poss = DevArray.from_host(poss)
        self.d_cloud_min, self.d_cloud_arg = DevArray((max(self.nc, 1),), np.float64), DevArray((max(self.nc, 1),), np.int32)
        # the raw clouds: global rows of their nearest sub-points, their labels (val_proj, val_labels)
        proj, raw_lab, self.raw_off = [], [], [0]
        for c, cl in enumerate(clouds):
            pi = cl.get("proj_idx")
            proj.append(self.off[c] + (np.arange(sizes[c]) if pi is None else np.asarray(pi, np.int64)))
            rl = cl.get("raw_labels") if pi is not None else cl.get("labels")
            raw_lab.append(None if rl is None else np.asarray(relabel(np.asarray(rl, np.int32)), np.int32))
            self.raw_off.append(self.raw_off[-1] + len(proj[-1]))
        self.n_raw = self.raw_off[-1]
        self.d_proj = DevArray.from_host(np.concatenate(proj).astype(np.int32)) if self.nc else None
        self.has_raw_labels = self.nc > 0 and all(r is not None and len(r) == len(p) for r, p in zip(raw_lab, proj))
        self._raw_labels = np.concatenate(raw_lab) if self.has_raw_labels else None
        self.test_probs = DevArray.from_host(np.zeros((self.n, self.C), np.float32))
        self.owner = DevArray.from_host(np.full(max(self.n, 1), -1, np.int32))
        self.net = randlanet.Network(cfg).load(weights).set_precision(precision)
        mk = lambda: (lambda p: (_lib.check(L.ssdr_stream_create(C.byref(p))), p.value)[1])(C.c_void_p())
        self.s_gen, self.s_up, self.s_net = mk(), mk(), mk()
        ev = lambda: (lambda p: (_lib.check(L.ssdr_event_create(C.byref(p))), p.value)[1])(C.c_void_p())
        N, B, K = self.N, self.B, cfg.k_n
        self.pads = bool(sizes) and min(sizes) < N            # the padding draws matter only when a cloud is smaller than a tile
        self.sets = []
        for _ in range(self.DEPTH):
            self.sets.append(dict(
                noise=DevArray((B, 3), np.float32), perm=DevArray((B, N), np.int32), dup=DevArray.from_host(np.zeros((B, N), np.float32)),
                xyz=DevArray((B, N, 3), np.float32), feat=DevArray((B, N, 6), np.float32), idx=DevArray((B, N), np.int32),
                labels=DevArray((B, N), np.int32) if self.has_labels else None, cloud=DevArray((B,), np.int32), center=DevArray((B, 3), np.float32),
                ready=ev(), consumed=ev(), gen_used=False, net_used=False))
            if sem:
                self.sets[-1].update(rot=DevArray((B, 2), np.float64), scale=DevArray((B, 3), np.float64),
                                     aug_noise=DevArray((B, N, 3), np.float64) if self.augment_noise != 0 else None)
        lv = [N]
        for r in cfg.sub_sampling_ratio:
            lv.append(lv[-1] // r)
        self.neigh = [DevArray((B, lv[i], K), np.int32) for i in range(cfg.num_layers)]
        self.interp = [DevArray((B, lv[i], 1), np.int32) for i in range(cfg.num_layers)]
        self.probs, self.f32 = DevArray((B * N, self.C), np.float32), DevArray((B * N, 32), np.float32)
        self.epochs, self.tiles, self.min_history = 0, 0, []
        self.confusion = self.ious = self.sub_confusion = self.sub_ious = None
        self._issued = self._done = 0            # batches whose generator / network has been enqueued
        self._step_in_epoch = 0
        if self.nc:
            _lib.check(L.ssdr_vote_init_dev(self.d_poss.ptr, _lib.ptr(self.off), self.nc, self.d_cloud_min.ptr, self.d_cloud_arg.ptr, self.s_gen))

    def close(self):
        L = _lib.lib()
        for s in (getattr(self, "s_gen", None), getattr(self, "s_up", None), getattr(self, "s_net", None)):
            if s:
                L.ssdr_stream_sync(s)
        for st in getattr(self, "sets", []):
            L.ssdr_event_destroy(st["ready"]); L.ssdr_event_destroy(st["consumed"])
        for s in ("s_gen", "s_up", "s_net"):
            if getattr(self, s, None):
                L.ssdr_stream_destroy(getattr(self, s)); setattr(self, s, None)
        self.sets = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- randomness (host; draws="device": the per-tile entries only) -----------------------------------------------------
    def draw(self, epoch, step):
        """the draws of one batch from (seed, epoch, step): noise [B,3] = normal(0, noise_init / 10) cast to float32 (test.py:114-115), one shuffle
        permutation per tile (DP.shuffle_idx, :125), the padding draws of data_aug (:137-141; zeros when no cloud is smaller than a tile).
        draws="device": the noise alone.  Semantic3D: also rot [B,2] = (cos, sin) of theta = uniform(0, 2 pi), scale [B,3] = uniform(scale_min,
        scale_max) times the symmetry signs and aug_noise float64 [B,N,3] = normal(0, augment_noise) (None when that is 0), as TrainFeeder.draw
        builds them (test3.py:220-256); draws="device": without aug_noise."""
        rng = np.random.default_rng([self.seed, int(epoch), int(step)])
        cfg, b = self.cfg, self.B
        host = self.draws == "host"
        d = dict(noise=rng.normal(scale=cfg.noise_init / 10, size=(b, 3)).astype(np.float32))
        if host:
            d.update(perm=np.stack([rng.permutation(self.N) for _ in range(b)]).astype(np.int32),
                     dup=rng.random((b, self.N), dtype=np.float32) if self.pads else None)
        if self.sem:
            theta = rng.uniform(0, 2 * np.pi, size=b)
            lo, hi = getattr(cfg, "augment_scale_min", 1.0), getattr(cfg, "augment_scale_max", 1.0)
            s = rng.uniform(lo, hi, size=(b, 3)) if getattr(cfg, "augment_scale_anisotropic", True) else np.repeat(rng.uniform(lo, hi, size=(b, 1)), 3, axis=1)
            sym = np.ones((b, 3))
            for i, on in enumerate(getattr(cfg, "augment_symmetries", [False, False, False])):
                if on:
                    sym[:, i] = np.round(rng.uniform(size=b)) * 2 - 1
            d.update(rot=np.stack([np.cos(theta), np.sin(theta)], axis=1), scale=s * sym)
            if host:
                d.update(aug_noise=rng.normal(scale=self.augment_noise, size=(b, self.N, 3)) if self.augment_noise != 0 else None)
        return d

    # ---- the two halves of a batch, both enqueue-only ---------------------------------------------------------------------
    def _generate(self, draws, epoch=None, step=None):
        """get_batch (test.py:97-151) of the next batch on the generator's stream, into buffer set (batch % DEPTH).  epoch, step: the counter of
        the per-row draws made on the device (default: the batch about to run)"""
        if self.nc == 0:
            raise ValueError("VoteTester: no clouds")
        L = _lib.lib()
        st = self.sets[self._issued % self.DEPTH]
        if st["gen_used"]:
            _lib.check(L.ssdr_stream_wait_event(self.s_up, st["ready"]))       # the draws of DEPTH batches ago have been read
        on_device = self.draws == "device"
        ups = [("noise", np.float32)] + ([("perm", np.int32)] if not on_device or draws.get("perm") is not None else [])
        ups += [("dup", np.float32)] if draws.get("dup") is not None else []
        if self.sem:
            ups += [("rot", np.float64), ("scale", np.float64)]
            if draws.get("aug_noise") is not None:
                if st["aug_noise"] is None:
                    raise ValueError("VoteTester: augmentation noise drawn, but the config's augment_noise is 0")
                ups.append(("aug_noise", np.float64))
        noisy = self.sem and draws.get("aug_noise") is not None
        for k, dt in ups:
            a = np.ascontiguousarray(draws[k], dt)
            assert a.shape == st[k].shape, (k, a.shape, st[k].shape)
            _lib.check(L.ssdr_memcpy_h2d_on(st[k].ptr, _lib.ptr(a), a.nbytes, self.s_up))      # waits for the upload stream alone
        if on_device:         # the per-row entries the dict does not hold: same stream as their last reader, no event
            epoch, step = self.epochs if epoch is None else epoch, self._step_in_epoch if step is None else step
            if draws.get("perm") is None:
                device_draws.perm(self.seed, epoch, step, self.B, self.N, out=st["perm"], stream=self.s_gen)
            if draws.get("dup") is None and self.pads:
                device_draws.uniform(self.seed, epoch, step, device_draws.DUP, self.B * self.N, out=st["dup"], stream=self.s_gen)
            if self.sem and not noisy and self.augment_noise != 0:
                device_draws.normal(self.seed, epoch, step, device_draws.AUG_NOISE, self.B * self.N * 3, scale=self.augment_noise, out=st["aug_noise"],
                                    stream=self.s_gen)
                noisy = True
        if st["net_used"]:
            _lib.check(L.ssdr_stream_wait_event(self.s_gen, st["consumed"]))   # the tile buffers' last reader
        if self.sem:
            # get_batch (test3.py:143-192): the chain's general form, x / y centred, global rows, queried_pt_weight = 1; then tf_map's augmentation
            _lib.check(L.ssdr_feed_chain_dev(self.d_points.ptr, self.d_colors.ptr, 3, self.d_labels.ptr if self.has_labels else None, self.d_poss.ptr,
                                             self.d_cloud_min.ptr, self.d_cloud_arg.ptr, _lib.ptr(self.off), self.nc, self.B, self.N,
                                             st["noise"].ptr, st["perm"].ptr, st["dup"].ptr, self.color_scale, st["xyz"].ptr, st["feat"].ptr, st["idx"].ptr,
                                             st["labels"].ptr if self.has_labels else None, st["cloud"].ptr, st["center"].ptr,
                                             1 | 2, None, 0, None, None, None, None, self.s_gen))          # SSDR_FEED_XY_ONLY | SSDR_FEED_GLOBAL_ROWS
            _lib.check(L.ssdr_feed_augment_dev(st["xyz"].ptr, self.B, self.N, st["rot"].ptr, st["scale"].ptr, st["aug_noise"].ptr if noisy else None, 3,
                                               st["feat"].ptr, self.s_gen))
            _lib.check(L.ssdr_event_record(st["ready"], self.s_gen))
            st["gen_used"] = True
            self._issued += 1
            return st
        _lib.check(L.ssdr_vote_tiles_dev(self.d_points.ptr, self.d_colors.ptr, 3, self.d_labels.ptr if self.has_labels else None, self.d_poss.ptr,
                                         self.d_cloud_min.ptr, self.d_cloud_arg.ptr, _lib.ptr(self.off), self.nc, self.B, self.N,
                                         st["noise"].ptr, st["perm"].ptr, st["dup"].ptr, 1.0 / 255.0, st["xyz"].ptr, st["feat"].ptr, st["idx"].ptr,
                                         st["labels"].ptr if self.has_labels else None, st["cloud"].ptr, st["center"].ptr, self.s_gen))
        _lib.check(L.ssdr_event_record(st["ready"], self.s_gen))
        st["gen_used"] = True
        self._issued += 1
        return st

    def _network(self):
        """pyramid, network and votes (RandLANet.py:319-334) of the oldest generated batch, on the network's stream"""
        L = _lib.lib()
        cfg, B, N = self.cfg, self.B, self.N
        st = self.sets[self._done % self.DEPTH]
        s = self.s_net
        _lib.check(L.ssdr_stream_wait_event(s, st["ready"]))
        arr = C.c_void_p * cfg.num_layers
        r = np.asarray(cfg.sub_sampling_ratio, np.int32)
        _lib.check(L.ssdr_knn_pyramid_dev(st["xyz"].ptr, B, N, cfg.num_layers, _lib.ptr(r), cfg.k_n, arr(*[a.ptr for a in self.neigh]), None,
                                          arr(*[a.ptr for a in self.interp]), s))
        self.net.infer_dev(B, N, st["feat"].ptr, st["xyz"].ptr, [a.ptr for a in self.neigh], [a.ptr for a in self.interp], self.probs.ptr, self.f32.ptr, s)
        # tile by tile, in batch order: a point in two tiles of the batch is smoothed twice (:330-334)
        for j in range(B):
            _lib.check(L.ssdr_vote_smooth_dev(self.test_probs.ptr, st["idx"].ptr + 4 * j * N, self.probs.ptr + 4 * j * N * self.C, N, self.C,
                                              self.test_smooth, self.owner.ptr, s))
        _lib.check(L.ssdr_event_record(st["consumed"], s))
        st["net_used"] = True
        self._done += 1
        self.tiles += B
        return st

    def _drain(self):
        while self._done < self._issued:
            self._network()

    def run_batch(self, draws=None):
        """One get_batch + network + votes, finished on return.  Returns the batch's device arrays (xyz, feat, idx, labels, cloud, center,
        probs): they are overwritten by the batch after the next."""
        self._drain()
        if draws is None:
            draws = self.draw(self.epochs, self._step_in_epoch)
        self._generate(draws, self.epochs, self._step_in_epoch)
        st = self._network()
        self._step_in_epoch += 1
        _lib.sync(self.s_gen)
        _lib.check(_lib.lib().ssdr_knn_status(self.s_net, None))
        return dict(xyz=st["xyz"], feat=st["feat"], idx=st["idx"], labels=st["labels"], cloud=st["cloud"], center=st["center"], probs=self.probs)

    def _epoch(self, draws=None):
        """val_steps batches; the generator runs ahead of the network by up to DEPTH batches.  Returns min(min_possibility) (:339)."""
        self._drain()
        gen = net = self._step_in_epoch
        while net < self.steps:
            while gen < self.steps and gen - net < self.DEPTH:
                self._generate(self.draw(self.epochs, gen) if draws is None else draws(self.epochs, gen), self.epochs, gen)
                gen += 1
            self._network()
            net += 1
        self._step_in_epoch = 0
        _lib.check(_lib.lib().ssdr_knn_status(self.s_net, None))               # what the enqueue-only pyramids could not report (waits for the network's stream)
        _lib.sync(self.s_gen)
        new_min = float(self.d_cloud_min.to_host(self.s_gen)[: self.nc].min())
        self.epochs += 1
        self.min_history.append(new_min)
        return new_min

    # ---- results -------------------------------------------------------------------------------------------------------
    def possibility(self):
        """the map, per cloud (host copies; waits for the generator)"""
        _lib.sync(self.s_gen)
        p = self.d_poss.to_host(self.s_gen)
        return [p[self.off[c]:self.off[c + 1]] for c in range(self.nc)]

    def cloud_state(self):
        """(min_possibility [C], local arg-min row [C]) (host copies; waits for the generator)"""
        _lib.sync(self.s_gen)
        return self.d_cloud_min.to_host(self.s_gen)[: self.nc], self.d_cloud_arg.to_host(self.s_gen)[: self.nc]

    def probs_host(self):
        _lib.sync(self.s_net)
        return self.test_probs.to_host(self.s_net)

    def _confusion(self, d_proj, labels, n, want_pred=False):
        d_l = labels if isinstance(labels, DevArray) else DevArray.from_host(np.ascontiguousarray(labels, np.int32), self.s_net)
        d_conf = DevArray.from_host(np.zeros((self.C, self.C), np.uint64), self.s_net); d_iou = DevArray((self.C,), np.float64)
        d_pred = DevArray((n,), np.int32) if want_pred else None
        _lib.check(_lib.lib().ssdr_confusion_dev(self.test_probs.ptr, self.C, d_proj.ptr if d_proj is not None else None, d_l.ptr, n,
                                                 d_pred.ptr if want_pred else None, d_conf.ptr, d_iou.ptr, self.s_net))
        _lib.sync(self.s_net)
        return d_conf.to_host(self.s_net).astype(np.int64), d_iou.to_host(self.s_net), (d_pred.to_host(self.s_net) if want_pred else None)

    def predictions(self):
        """per cloud: argmax(test_probs[proj_idx]) (:381-394); needs no labels"""
        if self.nc == 0:
            return []
        self._drain()
        _, _, pred = self._confusion(self.d_proj, np.full(self.n_raw, -1, np.int32), self.n_raw, want_pred=True)
        return [pred[self.raw_off[c]:self.raw_off[c + 1]] for c in range(self.nc)]

    def evaluate(self, max_epochs=None, draws=None):
        """The loop of RandLANet.py:305-424: whole epochs until the smallest possibility has grown by more than one vote, then the sub-cloud
        confusion rescaled by val_proportions (:353-368), the re-projected confusion, OA and m_IoU (:377-419).  Returns (m_IoU, OA);
        (0, 0) when max_epochs ends the loop first.  Semantic3D (SSRD_AL_semantic3d/RandLANet.py:351-485): more than vote_gap votes, last_min
        becomes new_min, OA = correct / seen over the rows that are not ignored; (m_IoU, 0) when num_votes or max_epochs ends the loop first.  draws: a callable (epoch, step) -> the batch's draws (see draw()) in place of the seeded ones."""
        if self.nc == 0:
            raise ValueError("VoteTester.evaluate: no clouds")
        if not (self.has_labels and self.has_raw_labels):
            raise ValueError("VoteTester.evaluate: every cloud needs labels (and raw_labels with proj_idx); predictions() works without")
        val_proportions = np.zeros(self.C, np.float32)                     # :298-303 (label_values = 0 .. C-1, none ignored)
        for i in range(self.C):
            val_proportions[i] = np.sum(self._raw_labels == i)
        last_min = -0.5
        m_iou, oa = 0, 0
        ran = 0
        while last_min < self.num_votes:
            if max_epochs is not None and ran >= max_epochs:
                break
            new_min = self._epoch(draws)
            ran += 1
            if last_min + self.vote_gap < new_min:
                last_min = new_min if self.sem else last_min + 1
                sub_conf, _, _ = self._confusion(None, self.d_labels, self.n)
                self.sub_confusion = sub_conf
                Cm = sub_conf.astype(np.float32)                                                       # :362
                Cm *= np.expand_dims(val_proportions / (np.sum(Cm, axis=1) + 1e-6), 1)     # :365
                self.sub_ious = _iou_host(Cm)
                conf, ious, _ = self._confusion(self.d_proj, self._raw_labels, self.n_raw)
                self.confusion, self.ious = conf, ious
                seen = int(np.sum(self._raw_labels != -1)) if self.sem else self.n_raw                 # len(labels_valid), :464
                oa = int(np.trace(conf)) / float(seen)                                                 # :398-408
                m_iou = float(np.mean(ious))                                                           # :411
                return m_iou, oa
        return m_iou, oa
