"""Training batches on the device: what Network.train() reads (the reference's ``input_list``), generated ahead of the consumer from the
resident clouds and the resident pseudo_gt.

S3DIS:      S3DIS_Dataset(mode="training") behind a shuffling DataLoader (the reference's SSDR_AL_s3dis/s3dis_dataset.py:115-193, main_S3DIS:
            every cloud once per epoch in a random order, batches of batch_size, the last one partial) -> ssdr_feed_tiles_dev.
Semantic3D: Semantic3D_Dataset_Train.get_batch (the reference's SSRD_AL_semantic3d/semantic3d_dataset_train.py:136-276: train_steps batches
            per epoch, the class-weighted possibility chain, x / y centring, tf_augment_input) -> ssdr_feed_chain_dev, ssdr_feed_augment_dev.
Both:       tf_map's pyramid (ssdr_knn_pyramid_dev with the pool outputs) on the generator's stream, the sub-sampled xyz levels copied out as the
            prefixes they are (ssdr_feed_prefix_dev).

The training step itself (forward, loss, backward, optimiser) is ``trainer.Trainer.step``."""
import ctypes as C

import numpy as np

from . import _lib
from . import draws as device_draws
from ._lib import DevArray

XY_ONLY, GLOBAL_ROWS = 1, 2          # SSDR_FEED_*


class _View(DevArray):
    """the leading rows of a DevArray (a partial batch): no buffer of its own"""

    def __init__(self, base, shape):
        self.shape, self.dtype, self.ptr, self._base = tuple(int(s) for s in shape), base.dtype, base.ptr, base
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        assert self.nbytes <= base.nbytes

    def __del__(self):
        pass


class FeedBatch:
    """One batch: ``arrays`` is the reference's input_list (s3dis_dataset.py:180-181) as device arrays,
    [xyz_0 .. xyz_L-1, neigh_0 .., pool_0 .., up_0 .., features, labels, activation, pseudo, pc_idx, cloud_idx].
    The consumer's stream was told to wait for the batch when it was handed out; ``release(stream)`` gives the buffers back
    once that stream's work so far has run.  They are overwritten DEPTH batches later."""

    def __init__(self, feeder, st, arrays, size, epoch, step):
        self._feeder, self._st, self.arrays, self.size, self.epoch, self.step = feeder, st, arrays, size, epoch, step
        self.center = _View(st["center"], (size, 3))
        self.released = False

    def __getitem__(self, i):
        return self.arrays[i]

    def __len__(self):
        return len(self.arrays)

    def wait(self, stream):
        """make another stream wait for the batch as well"""
        _lib.check(_lib.lib().ssdr_stream_wait_event(stream, self._st["ready"]))

    def release(self, stream=None):
        if self.released:
            return
        self.released = True
        self._feeder._release(self._st, stream)

    def to_host(self):
        """the NumPy input_list (waits for the generator)"""
        _lib.sync(self._feeder.s_gen)
        return [a.to_host(self._feeder.s_gen) for a in self.arrays]


class TrainFeeder:
    """``clouds[c]`` = dict(xyz [n,3], rgb [n,3], labels [n]): the sub-sampled training clouds, concatenated on the device.

    ``pseudo_gt``: a list of per-cloud float32 [2, n_c] arrays (row 0 the activation mask, row 1 the pseudo label: what io_formats reads from a
    round's .gt files), or a pair of device arrays float32 [sum n_c] over the clouds' concatenation, e.g. ``(LabelResult.mask, LabelResult.label)``
    of an ALRound whose ``HotPath.pt_off`` equals this feeder's ``off``.  The pair is used in place: a batch generated after the next labelling
    reads what that labelling wrote.

    The host draws the randomness from (seed, epoch, step) (``draw``, replaceable); the generator runs on a stream of its own, at most DEPTH
    batches ahead of the consumer; draws are uploaded on a third stream.  Every buffer set has two kinds of arrays.  The draw buffers (noise, shuffle,
    padding draws, S3DIS tile cloud / point, Semantic3D rotation / scale / augmentation noise) are written by the upload stream and read by the generator
    alone: the upload stream waits for the set's previous ``ready`` event before it overwrites them.  The batch arrays (everything a FeedBatch hands out,
    cloud_idx and the centres included) are written by the generator alone: its stream waits for the set's ``consumed`` event first, so nothing a consumer
    may still read is touched before the consumer's stream has run what it had enqueued at ``release``.  ``next_batch(stream)`` hands out the oldest generated batch (None at
    the end of an epoch); ``for batch in feeder.epoch_batches(stream)`` does the same.

    ``draws="device"``: the per-row draws (shuffle permutations, padding draws, augmentation noise) are made on the device from the counter
    (seed, epoch, step, kind, element) instead (``ssdr_al.draws``); ``draw`` then returns the per-tile entries alone and nothing
    per row is uploaded.  The rule is per key: a per-row entry that a ``draws=`` callable does return is uploaded.  A draw made on the device needs
    no event of its own: it is enqueued on the generator's stream in front of the chain, the stream whose chain was the last reader of those
    buffers, and the set's next upload waits for ``ready`` as before."""

    DEPTH = 2

    def __init__(self, clouds, pseudo_gt, config=None, dataset="S3DIS", seed=0, possibility=None, class_weight=None, color_scale=1.0, draws="host"):
        from .helper_tool import ConfigS3DIS, ConfigSemantic3D
        if draws not in ("host", "device"):
            raise ValueError("TrainFeeder: draws must be 'host' or 'device'")
        self.draws = draws
        if dataset not in ("S3DIS", "Semantic3D"):
            raise ValueError("TrainFeeder: dataset must be 'S3DIS' or 'Semantic3D'")
        self.dataset = dataset
        cfg = self.cfg = (ConfigS3DIS if dataset == "S3DIS" else ConfigSemantic3D) if config is None else config
        self.nc = len(clouds)
        if self.nc == 0:
            raise ValueError("TrainFeeder: no clouds")
        self.seed, self.color_scale = int(seed), float(color_scale)
        self.N, self.B, self.K, self.L = int(cfg.num_points), int(cfg.batch_size), int(cfg.k_n), int(cfg.num_layers)
        self.train_steps = int(getattr(cfg, "train_steps", 500))
        sizes = self.sizes = [len(c["xyz"]) for c in clouds]
        if min(sizes) <= 0:
            raise ValueError("TrainFeeder: an empty cloud")
        if dataset == "Semantic3D" and min(sizes) < self.N:
            raise ValueError("TrainFeeder: a Semantic3D cloud of %d points is smaller than num_points = %d (the reference's tree query raises there)"
                             % (min(sizes), self.N))
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n = int(self.off[-1])
        L = _lib.lib()
        _lib.check(L.ssdr_init(0))
        cat = lambda key, dt, w: np.concatenate([np.asarray(c[key], dt).reshape(len(c["xyz"]), *w) for c in clouds])
        labels = cat("labels", np.int32, ())
        self.d_points = DevArray.from_host(cat("xyz", np.float32, (3,)))
        self.d_colors = DevArray.from_host(cat("rgb", np.float32, (3,)))
        self.d_labels = DevArray.from_host(labels)
        if isinstance(pseudo_gt, (tuple, list)) and len(pseudo_gt) == 2 and all(isinstance(p, DevArray) for p in pseudo_gt):
            act, pse = pseudo_gt
            for p in (act, pse):
                if p.dtype != np.float32 or int(np.prod(p.shape)) != self.n:
                    raise ValueError("TrainFeeder: the device pseudo_gt pair must be float32 [%d], one entry per point of the concatenated clouds" % self.n)
            self.d_act, self.d_pse = act, pse                           # in place: no copy
        else:
            if len(pseudo_gt) != self.nc:
                raise ValueError("TrainFeeder: one pseudo_gt per cloud")
            pg = [np.asarray(p, np.float32) for p in pseudo_gt]
            for p, n in zip(pg, sizes):
                if p.shape != (2, n):
                    raise ValueError("TrainFeeder: pseudo_gt of a cloud of %d points must be [2, %d]" % (n, n))
            self.d_act = DevArray.from_host(np.concatenate([p[0] for p in pg]))
            self.d_pse = DevArray.from_host(np.concatenate([p[1] for p in pg]))
        # RandLANet.py:232 (S3DIS; len(dataset) = the clouds)
        self.one_epoch_steps = int(self.B * self.train_steps / self.nc + 1)
        self.steps_per_epoch = (self.nc + self.B - 1) // self.B if dataset == "S3DIS" else self.train_steps
        mk = lambda: (lambda p: (_lib.check(L.ssdr_stream_create(C.byref(p))), p.value)[1])(C.c_void_p())
        self.s_gen, self.s_up = mk(), mk()
        ev = lambda: (lambda p: (_lib.check(L.ssdr_event_create(C.byref(p))), p.value)[1])(C.c_void_p())
        N, B, K = self.N, self.B, self.K
        self.pads = min(sizes) < N
        lv = self.level_rows = [N]
        for r in cfg.sub_sampling_ratio[: self.L]:
            lv.append(lv[-1] // r)
        sem = dataset == "Semantic3D"
        self.augment_noise = float(getattr(cfg, "augment_noise", 0.0)) if sem else 0.0
        self.sets = []
        for _ in range(self.DEPTH):
            st = dict(noise=DevArray((B, 3), np.float32), perm=DevArray((B, N), np.int32), dup=DevArray.from_host(np.zeros((B, N), np.float32)),
                      xyz=[DevArray((B, lv[i], 3), np.float32) for i in range(self.L)],
                      neigh=[DevArray((B, lv[i], K), np.int32) for i in range(self.L)], pool=[DevArray((B, lv[i + 1], K), np.int32) for i in range(self.L)],
                      up=[DevArray((B, lv[i], 1), np.int32) for i in range(self.L)],
                      feat=DevArray((B, N, 6), np.float32), labels=DevArray((B, N), np.int32), act=DevArray((B, N), np.float32), pse=DevArray((B, N), np.float32),
                      idx=DevArray((B, N), np.int32), cloud=DevArray((B,), np.int32), center=DevArray((B, 3), np.float32),
                      ready=ev(), consumed=ev(), gen_used=False, held=False, wait_consumed=False)
            if sem:
                st.update(rot=DevArray((B, 2), np.float64), scale=DevArray((B, 3), np.float64),
                          aug_noise=DevArray((B, N, 3), np.float64) if self.augment_noise != 0 else None)
            else:
                st.update(tile_cloud=DevArray((B,), np.int32), point=DevArray((B,), np.int32))      # draws: never handed out (cloud_idx is written by the generator)
            self.sets.append(st)
        self.epoch, self._gen_step, self._out_step, self._queue, self._issued, self._draws = 0, 0, 0, [], 0, None
        if sem:
            if possibility is None:
                possibility = [np.random.default_rng([self.seed, c]).random(n) * 1e-3 for c, n in enumerate(sizes)]      # init_possibility, :144-146
            self.d_poss = DevArray.from_host(np.concatenate([np.asarray(p, np.float64) for p in possibility]))
            if class_weight is None:
                _, num_class_total = np.unique(labels, return_counts=True)                                               # :148-149
                class_weight = num_class_total / np.sum(num_class_total)
            self.class_weight = np.ascontiguousarray(class_weight, np.float64).reshape(-1)
            if labels.min() < 0 or labels.max() >= len(self.class_weight):
                # the reference maps labels through label_to_idx first (:186); here they index the weights as they are
                raise ValueError("TrainFeeder: labels span %d .. %d but there are %d class weights: labels must be 0 .. len(class_weight) - 1 "
                                 "(remap them, or pass class_weight with one entry per label value)" % (labels.min(), labels.max(), len(self.class_weight)))
            self.d_cw = DevArray.from_host(self.class_weight)
            self.d_cloud_min, self.d_cloud_arg = DevArray((self.nc,), np.float64), DevArray((self.nc,), np.int32)
            _lib.check(L.ssdr_vote_init_dev(self.d_poss.ptr, _lib.ptr(self.off), self.nc, self.d_cloud_min.ptr, self.d_cloud_arg.ptr, self.s_gen))

    def close(self):
        L = _lib.lib()
        for s in (getattr(self, "s_gen", None), getattr(self, "s_up", None)):
            if s:
                L.ssdr_stream_sync(s)
        for st in getattr(self, "sets", []):
            L.ssdr_event_destroy(st["ready"]); L.ssdr_event_destroy(st["consumed"])
        for s in ("s_gen", "s_up"):
            if getattr(self, s, None):
                L.ssdr_stream_destroy(getattr(self, s)); setattr(self, s, None)
        self.sets = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- randomness (host; draws="device": the per-tile entries only) -----------------------------------------------------
    def order(self, epoch):
        """S3DIS: the DataLoader's permutation of the clouds for this epoch"""
        return np.random.default_rng([self.seed, int(epoch)]).permutation(self.nc).astype(np.int32)

    def batch_size_of(self, step):
        return min(self.B, self.nc - step * self.B) if self.dataset == "S3DIS" else self.B

    def draw(self, epoch, step):
        """The draws of one batch from (seed, epoch, step).  Both: noise [b,3] = normal(0, noise_init / 10) cast to float32, one shuffle permutation
        per tile, the padding draws (None when no cloud is smaller than a tile).  S3DIS: cloud [b] (the epoch's order) and point [b] = randint(n_c)
        (s3dis_dataset.py:119).  Semantic3D: rot [b,2] = (cos, sin) of theta = uniform(0, 2 pi), scale [b,3] = uniform(scale_min, scale_max) (one
        value for all axes unless anisotropic) times the symmetry signs, aug_noise float64 [b,N,3] = normal(0, augment_noise) or None when that is 0
        (semantic3d_dataset_train.py:240-272).  draws="device": without perm, dup and aug_noise."""
        rng = np.random.default_rng([self.seed, int(epoch), int(step)])
        b, N, cfg = self.batch_size_of(step), self.N, self.cfg
        host = self.draws == "host"
        d = dict(noise=rng.normal(scale=cfg.noise_init / 10, size=(b, 3)).astype(np.float32))
        if host:
            d.update(perm=np.stack([rng.permutation(N) for _ in range(b)]).astype(np.int32),
                     dup=rng.random((b, N), dtype=np.float32) if self.pads else None)
        if self.dataset == "S3DIS":
            cloud = self.order(epoch)[step * self.B: step * self.B + b]
            d.update(cloud=cloud, point=np.array([rng.integers(0, self.sizes[c]) for c in cloud], np.int32))
        else:
            theta = rng.uniform(0, 2 * np.pi, size=b)
            lo, hi = getattr(cfg, "augment_scale_min", 1.0), getattr(cfg, "augment_scale_max", 1.0)
            s = rng.uniform(lo, hi, size=(b, 3)) if getattr(cfg, "augment_scale_anisotropic", True) else np.repeat(rng.uniform(lo, hi, size=(b, 1)), 3, axis=1)
            sym = np.ones((b, 3))
            for i, on in enumerate(getattr(cfg, "augment_symmetries", [False, False, False])):
                if on:
                    sym[:, i] = np.round(rng.uniform(size=b)) * 2 - 1
            d.update(rot=np.stack([np.cos(theta), np.sin(theta)], axis=1), scale=s * sym)
            if host:
                d.update(aug_noise=rng.normal(scale=self.augment_noise, size=(b, N, 3)) if self.augment_noise != 0 else None)
        return d

    # ---- the generator: enqueue only --------------------------------------------------------------------------------------
    def _generate(self, draws, epoch, step):
        L = _lib.lib()
        st = self.sets[self._issued % self.DEPTH]
        b, N = len(draws["noise"]), self.N
        if st["gen_used"]:
            _lib.check(L.ssdr_stream_wait_event(self.s_up, st["ready"]))       # the draws of DEPTH batches ago have been read
        on_device = self.draws == "device"
        ups = [("noise", np.float32)] + ([("perm", np.int32)] if not on_device or draws.get("perm") is not None else [])
        ups += [("dup", np.float32)] if draws.get("dup") is not None else []
        ups += [("tile_cloud", np.int32), ("point", np.int32)] if self.dataset == "S3DIS" else [("rot", np.float64), ("scale", np.float64)]
        if draws.get("aug_noise") is not None:
            if st.get("aug_noise") is None:
                raise ValueError("TrainFeeder: augmentation noise drawn, but the config's augment_noise is 0")
            ups.append(("aug_noise", np.float64))
        for k, dt in ups:
            a = np.ascontiguousarray(draws["cloud" if k == "tile_cloud" else k], dt)
            assert a.shape == (b,) + st[k].shape[1:], (k, a.shape, st[k].shape)
            _lib.check(L.ssdr_memcpy_h2d_on(st[k].ptr, _lib.ptr(a), a.nbytes, self.s_up))      # waits for the upload stream alone
        noisy = draws.get("aug_noise") is not None
        if on_device:         # the per-row entries the dict does not hold: same stream as their last reader, no event
            if draws.get("perm") is None:
                device_draws.perm(self.seed, epoch, step, b, N, out=st["perm"], stream=self.s_gen)
            if draws.get("dup") is None and self.pads:
                device_draws.uniform(self.seed, epoch, step, device_draws.DUP, b * N, out=st["dup"], stream=self.s_gen)
            if not noisy and self.augment_noise != 0:
                device_draws.normal(self.seed, epoch, step, device_draws.AUG_NOISE, b * N * 3, scale=self.augment_noise, out=st["aug_noise"], stream=self.s_gen)
                noisy = True
        if st["wait_consumed"]:
            _lib.check(L.ssdr_stream_wait_event(self.s_gen, st["consumed"]))   # the buffers' last reader
            st["wait_consumed"] = False
        s = self.s_gen
        xyz0 = st["xyz"][0]
        if self.dataset == "S3DIS":
            _lib.check(L.ssdr_feed_tiles_dev(self.d_points.ptr, self.d_colors.ptr, 3, self.d_labels.ptr, self.d_act.ptr, self.d_pse.ptr, _lib.ptr(self.off), self.nc,
                                             b, N, st["tile_cloud"].ptr, st["point"].ptr, st["noise"].ptr, st["perm"].ptr, st["dup"].ptr, self.color_scale,
                                             xyz0.ptr, st["feat"].ptr, st["idx"].ptr, st["labels"].ptr, st["act"].ptr, st["pse"].ptr, st["cloud"].ptr, st["center"].ptr, s))
        else:
            _lib.check(L.ssdr_feed_chain_dev(self.d_points.ptr, self.d_colors.ptr, 3, self.d_labels.ptr, self.d_poss.ptr, self.d_cloud_min.ptr, self.d_cloud_arg.ptr,
                                             _lib.ptr(self.off), self.nc, b, N, st["noise"].ptr, st["perm"].ptr, st["dup"].ptr, self.color_scale,
                                             xyz0.ptr, st["feat"].ptr, st["idx"].ptr, st["labels"].ptr, st["cloud"].ptr, st["center"].ptr,
                                             XY_ONLY, self.d_cw.ptr, len(self.class_weight), self.d_act.ptr, self.d_pse.ptr, st["act"].ptr, st["pse"].ptr, s))
            an = st["aug_noise"].ptr if noisy else None
            _lib.check(L.ssdr_feed_augment_dev(xyz0.ptr, b, N, st["rot"].ptr, st["scale"].ptr, an, 3, st["feat"].ptr, s))
        arr = C.c_void_p * self.L
        r = np.asarray(self.cfg.sub_sampling_ratio[: self.L], np.int32)
        _lib.check(L.ssdr_knn_pyramid_dev(xyz0.ptr, b, N, self.L, _lib.ptr(r), self.K, arr(*[a.ptr for a in st["neigh"]]), arr(*[a.ptr for a in st["pool"]]),
                                          arr(*[a.ptr for a in st["up"]]), s))
        for i in range(1, self.L):
            _lib.check(L.ssdr_feed_prefix_dev(xyz0.ptr, b, N, self.level_rows[i], st["xyz"][i].ptr, s))
        _lib.check(L.ssdr_event_record(st["ready"], s))
        st["gen_used"], st["held"] = True, True
        v = lambda a: a if b == self.B else _View(a, (b,) + a.shape[1:])
        arrays = [v(a) for a in st["xyz"] + st["neigh"] + st["pool"] + st["up"]] + [v(st[k]) for k in ("feat", "labels", "act", "pse", "idx", "cloud")]
        self._queue.append(FeedBatch(self, st, arrays, b, epoch, step))

    def _top_up(self, draws=None):
        """generate while there is a batch of this epoch left, fewer than DEPTH are out, and the next buffer set has been released"""
        while self._gen_step < self.steps_per_epoch:
            if self.sets[self._issued % self.DEPTH]["held"]:
                break
            d = self.draw(self.epoch, self._gen_step) if draws is None else draws(self.epoch, self._gen_step)
            self._generate(d, self.epoch, self._gen_step)
            self._issued += 1
            self._gen_step += 1

    def _release(self, st, stream):
        _lib.check(_lib.lib().ssdr_event_record(st["consumed"], stream))
        st["held"], st["wait_consumed"] = False, True
        self._top_up(self._draws)

    def next_batch(self, stream=None, draws=None):
        """The next batch of the epoch, or None when the epoch is over (the call after that starts the next one).  ``stream`` (the consumer's; None:
        the library's) is told to wait for the batch.  draws: a callable (epoch, step) -> the batch's draws in place of ``draw``."""
        L = _lib.lib()
        self._draws = draws
        if self._out_step >= self.steps_per_epoch:
            self.epoch += 1
            self._gen_step = self._out_step = 0
            self.check()
            return None
        self._top_up(draws)
        if not self._queue:
            raise RuntimeError("TrainFeeder: all %d buffer sets are held: release() a batch before asking for the next" % self.DEPTH)
        batch = self._queue.pop(0)
        _lib.check(L.ssdr_stream_wait_event(stream, batch._st["ready"]))
        self._out_step += 1
        return batch

    def epoch_batches(self, stream=None, draws=None):
        """one epoch's batches; each is released on ``stream`` when the next one is asked for, unless the caller has done so"""
        while True:
            batch = self.next_batch(stream, draws)
            if batch is None:
                return
            yield batch
            batch.release(stream)

    def check(self):
        """what the enqueue-only calls could not report (waits for the generator): the pyramid's capacities, the feed's status bits"""
        L = _lib.lib()
        _lib.check(L.ssdr_knn_status(self.s_gen, None))
        _lib.check(L.ssdr_feed_status(self.s_gen, None))

    # ---- Semantic3D state ---------------------------------------------------------------------------------------------------
    def possibility(self):
        """the map, per cloud (host copies; waits for the generator)"""
        _lib.sync(self.s_gen)
        p = self.d_poss.to_host(self.s_gen)
        return [p[self.off[c]:self.off[c + 1]] for c in range(self.nc)]

    def cloud_state(self):
        _lib.sync(self.s_gen)
        return self.d_cloud_min.to_host(self.s_gen), self.d_cloud_arg.to_host(self.s_gen)
