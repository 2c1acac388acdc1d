"""Training batches on the device (ssdr_feed_chain_dev / ssdr_feed_tiles_dev / ssdr_feed_augment_dev, ssdr_al.training.TrainFeeder) against the NumPy
restatement of the reference's two training generators (tests/_feed_oracle.py).

Shapes: num_points 1024 over clouds of 300 (padded), 1024, 1029, 2117 and 5000 points.  Every comparison is index for index and bit for bit; the one
exception (the restated augment against the reference's np.matmul form, whose BLAS may fuse) is bounded by one float32 ulp and its count printed."""
import numpy as np
import pytest

import _feed_oracle as FO
import _vote_oracle as VO
from conftest import assert_bits_equal

N = 1024
SSDR_ERR_INVALID, SSDR_ERR_UNSUPPORTED = 1, 5
XY_ONLY, GLOBAL_ROWS = 1, 2
SCALE = np.float32(1.0 / 255.0)


class _Dev:
    """the clouds, channels and (optionally) the map on the device; one call of each generator through the C ABI"""

    def __init__(self, clouds, acts, pses, poss=None, num_points=N):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        _lib.check(_lib.lib().ssdr_init(0))
        self.nc, self.N = len(clouds), int(num_points)
        self.off = np.concatenate([[0], np.cumsum([len(c["xyz"]) for c in clouds])]).astype(np.int64)
        self.d_p = DevArray.from_host(np.concatenate([c["xyz"] for c in clouds]))
        self.d_c = DevArray.from_host(np.concatenate([c["rgb"] for c in clouds]).astype(np.float32))
        self.d_l = DevArray.from_host(np.concatenate([c["labels"] for c in clouds]).astype(np.int32))
        self.d_a = DevArray.from_host(np.concatenate(acts).astype(np.float32))
        self.d_s = DevArray.from_host(np.concatenate(pses).astype(np.float32))
        if poss is not None:
            self.d_poss = DevArray.from_host(np.concatenate(poss))
            self.d_min, self.d_arg = DevArray((self.nc,), np.float64), DevArray((self.nc,), np.int32)
            _lib.check(_lib.lib().ssdr_vote_init_dev(self.d_poss.ptr, _lib.ptr(self.off), self.nc, self.d_min.ptr, self.d_arg.ptr, None))

    @staticmethod
    def outputs(B, n=N):
        from ssdr_al._lib import DevArray
        return dict(xyz=DevArray((B, n, 3), np.float32), feat=DevArray((B, n, 6), np.float32), idx=DevArray((B, n), np.int32), labels=DevArray((B, n), np.int32),
                    act=DevArray((B, n), np.float32), pse=DevArray((B, n), np.float32), cloud=DevArray((B,), np.int32), center=DevArray((B, 3), np.float32))

    def chain(self, draws, flags, weights=None, channels=True, entry="feed"):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        L = _lib.lib()
        B = len(draws["noise"])
        assert draws["perm"].shape == (B, self.N) and draws["dup"].shape == (B, self.N)
        d_n, d_perm, d_dup = DevArray.from_host(draws["noise"]), DevArray.from_host(draws["perm"]), DevArray.from_host(draws["dup"])
        o = self.outputs(B, self.N)
        head = (self.d_p.ptr, self.d_c.ptr, 3, self.d_l.ptr, self.d_poss.ptr, self.d_min.ptr, self.d_arg.ptr, _lib.ptr(self.off), self.nc, B, self.N, d_n.ptr, d_perm.ptr,
                d_dup.ptr, float(SCALE), o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr, o["labels"].ptr, o["cloud"].ptr, o["center"].ptr)
        if entry == "vote":
            _lib.check(L.ssdr_vote_tiles_dev(*head, None))
        else:
            d_w = None if weights is None else DevArray.from_host(np.ascontiguousarray(weights, np.float64))
            _lib.check(L.ssdr_feed_chain_dev(*head, flags, d_w.ptr if d_w else None, 0 if weights is None else len(weights),
                                             self.d_a.ptr if channels else None, self.d_s.ptr if channels else None,
                                             o["act"].ptr if channels else None, o["pse"].ptr if channels else None, None))
        _lib.sync()
        return {k: v.to_host() for k, v in o.items() if channels or k not in ("act", "pse")}

    def tiles(self, tile_cloud, tile_point, draws):
        from ssdr_al import _lib
        from ssdr_al._lib import DevArray
        B = len(tile_cloud)
        assert draws["perm"].shape == (B, self.N) and draws["dup"].shape == (B, self.N)
        d_tc, d_tp = DevArray.from_host(np.asarray(tile_cloud, np.int32)), DevArray.from_host(np.asarray(tile_point, np.int32))
        d_n, d_perm, d_dup = DevArray.from_host(draws["noise"]), DevArray.from_host(draws["perm"]), DevArray.from_host(draws["dup"])
        o = self.outputs(B, self.N)
        _lib.check(_lib.lib().ssdr_feed_tiles_dev(self.d_p.ptr, self.d_c.ptr, 3, self.d_l.ptr, self.d_a.ptr, self.d_s.ptr, _lib.ptr(self.off), self.nc, B, self.N,
                                                  d_tc.ptr, d_tp.ptr, d_n.ptr, d_perm.ptr, d_dup.ptr, float(SCALE), o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr,
                                                  o["labels"].ptr, o["act"].ptr, o["pse"].ptr, o["cloud"].ptr, o["center"].ptr, None))
        _lib.sync()
        return {k: v.to_host() for k, v in o.items()}

    def state(self):
        return self.d_poss.to_host(), self.d_min.to_host(), self.d_arg.to_host()


def _channels(clouds, seed=5):
    r = np.random.default_rng(seed)
    acts = [(r.random(len(c["xyz"])) < 0.3).astype(np.float32) for c in clouds]
    pses = [r.integers(0, 8, len(c["xyz"])).astype(np.float32) for c in clouds]
    return acts, pses


def _compare(got, ref, what, keys=("center", "idx", "xyz", "feat", "labels", "act", "pse")):
    for k in keys:
        if k in ("idx", "labels", "cloud"):
            assert np.array_equal(got[k], ref[k]), what + " " + k
        else:
            assert_bits_equal(got[k], ref[k], what + " " + k)


# ---- 1. the weighted chain ------------------------------------------------------------------------------------------------------------
def _weighted_case():
    clouds, poss, rng = VO.make_case([1024, 1029, 2117, 5000])
    r = np.random.default_rng(11)
    for c in clouds:
        c["labels"] = r.integers(0, 8, len(c["xyz"])).astype(np.int32)
    clouds[3]["labels"][:3000] = 4
    _, cnt = np.unique(np.concatenate([c["labels"] for c in clouds]), return_counts=True)
    weights = cnt / np.sum(cnt)                                            # the reference's class_weight (:148-149): class frequencies
    poss = VO.add_ties(poss)
    acts, pses = _channels(clouds)
    return clouds, poss, rng, weights, acts, pses


@pytest.fixture(scope="module")
def weighted_reference():
    clouds, poss, rng, weights, acts, pses = _weighted_case()
    rng_perm = np.random.default_rng(99)
    gen = FO.ChainGenerator(clouds, poss, N, SCALE, xy_only=True, global_rows=False, class_weight=weights, activation=acts, pseudo=pses)
    plain = FO.ChainGenerator(clouds, poss, N, SCALE, xy_only=True, global_rows=False, activation=acts, pseudo=pses)
    draws, batches, states, plain_order = [], [], [], []
    for _ in range(3):
        d = VO.draw_batch(rng, rng_perm, 20, N)
        draws.append(d); batches.append(gen.batch(d)); plain_order.append(plain.batch(d)["cloud"])
        states.append((np.concatenate(gen.possibility).copy(), np.asarray(gen.min_possibility).copy(), gen.cloud_arg()))
    return clouds, poss, weights, acts, pses, draws, batches, states, np.concatenate(plain_order)


def test_weighted_chain(backend, weighted_reference):
    clouds, poss, weights, acts, pses, draws, batches, states, plain_order = weighted_reference
    # what the restatement alone says about these 60 tiles
    order = np.concatenate([b["cloud"] for b in batches])
    assert len(weights) == 8 and weights[4] > 0.3
    assert set(order.tolist()) == {0, 1, 2, 3}
    assert (order[1:] == order[:-1]).any()                               # a cloud visited in consecutive tiles: tile t + 1 reads tile t's minimum
    assert states[-1][0].min() >= 1e-3                                   # every row covered
    assert not np.array_equal(order, plain_order)                        # the weights decide the visit order: ignoring them cannot pass
    dev = _Dev(clouds, acts, pses, poss)
    for k in range(3):
        got = dev.chain(draws[k], XY_ONLY, weights)
        ref = batches[k]
        assert np.array_equal(got["cloud"], ref["cloud"]), "batch %d cloud ids" % k
        _compare(got, ref, "batch %d" % k)
        o = dev.off[ref["cloud"]]
        zsrc = np.concatenate([c["xyz"] for c in clouds])[(o[:, None] + ref["idx"])][..., 2]
        assert_bits_equal(got["xyz"][..., 2], zsrc, "batch %d: z is not centred" % k)
        assert ref["idx"].max() < 5000 and (ref["idx"] >= 0).all()       # cloud-local rows
        st = dev.state()
        assert np.array_equal(st[0], states[k][0]), "batch %d possibility map (float64, bit for bit)" % k
        assert np.array_equal(st[1], states[k][1]) and np.array_equal(st[2], states[k][2]), "batch %d cloud minima / arg-minima" % k
    from ssdr_al import _lib
    status = np.zeros(1, np.int32)
    assert _lib.lib().ssdr_feed_status(None, _lib.ptr(status)) == 0 and status[0] == 0
    # a label outside the weights: weight 0 and the status bit (the reference raises IndexError there)
    got = dev.chain(draws[0], XY_ONLY, weights[:4])
    assert _lib.lib().ssdr_feed_status(None, _lib.ptr(status)) == SSDR_ERR_INVALID and status[0] == 1
    assert _lib.lib().ssdr_feed_status(None, _lib.ptr(status)) == 0 and status[0] == 0      # read once


# ---- 2. the general entry reproduces ssdr_vote_tiles_dev ------------------------------------------------------------------------------
def test_chain_generality(backend):
    clouds, poss, rng = VO.make_case([300, 1024, 1029, 2117, 5000])
    poss = VO.add_ties(poss)
    acts, pses = _channels(clouds)
    rng_perm = np.random.default_rng(99)
    a, b = _Dev(clouds, acts, pses, poss), _Dev(clouds, acts, pses, poss)
    for k in range(3):
        d = VO.draw_batch(rng, rng_perm, 20, N)
        ga = a.chain(d, GLOBAL_ROWS, channels=False)
        gb = b.chain(d, 0, entry="vote", channels=False)
        assert (gb["cloud"] == 0).any() or k > 0                         # the 300-point cloud (padded) is among the first batch's tiles
        for key in ("cloud", "idx", "labels"):
            assert np.array_equal(ga[key], gb[key]), "batch %d %s" % (k, key)
        for key in ("center", "xyz", "feat"):
            assert_bits_equal(ga[key], gb[key], "batch %d %s" % (k, key))
        sa, sb = a.state(), b.state()
        assert all(np.array_equal(x, y) for x, y in zip(sa, sb)), "batch %d state" % k


# ---- 3. independent tiles ---------------------------------------------------------------------------------------------------------------
def test_independent_tiles(backend):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    clouds, _, rng = VO.make_case([300, 1024, 1029, 5000])
    acts, pses = _channels(clouds)
    tile_cloud = np.array([3, 1, 0, 2, 3, 1, 2], np.int32)               # clouds 1, 2, 3 twice, the padded cloud once
    tile_point = np.array([rng.integers(0, len(clouds[c]["xyz"])) for c in tile_cloud], np.int32)
    d = VO.draw_batch(rng, np.random.default_rng(3), 7, N)
    ref = FO.indep_batch(clouds, acts, pses, tile_cloud, tile_point, d, N, SCALE)
    dev = _Dev(clouds, acts, pses)
    got = dev.tiles(tile_cloud, tile_point, d)
    _compare(got, ref, "tiles")
    assert np.array_equal(got["cloud"], tile_cloud)                      # the ids, copied out in stream order
    # the channels' rows follow idx, the padding duplicates of the 300-point cloud included
    assert len(np.unique(got["idx"][2])) == 300
    for t, c in enumerate(tile_cloud):
        assert_bits_equal(got["act"][t], acts[c][got["idx"][t]], "tile %d activation" % t)
        assert_bits_equal(got["pse"][t], pses[c][got["idx"][t]], "tile %d pseudo" % t)
    # the batch entry fed the same centres: one tile per cloud, in order, so one call per tile here
    L = _lib.lib()
    for t, c in enumerate(tile_cloud):
        n = len(clouds[c]["xyz"])
        o = int(dev.off[c])
        off1 = np.array([0, n], np.int64)
        d_m = DevArray.from_host(np.array([n, 0], np.int64))
        d_perm, d_dup = DevArray.from_host(d["perm"][t]), DevArray.from_host(d["dup"][t])
        out = _Dev.outputs(1)
        center = np.ascontiguousarray(got["center"][t])
        _lib.check(L.ssdr_tile_select_batch_dev(dev.d_p.ptr + 12 * o, dev.d_c.ptr + 12 * o, 3, d_m.ptr, _lib.ptr(off1), 1, _lib.ptr(center), N, d_perm.ptr, d_dup.ptr,
                                                float(SCALE), out["xyz"].ptr, out["feat"].ptr, out["idx"].ptr, dev.d_l.ptr + 4 * o, out["labels"].ptr, None))
        _lib.sync()
        assert np.array_equal(got["idx"][t], out["idx"].to_host()[0]) and np.array_equal(got["labels"][t], out["labels"].to_host()[0]), "tile %d rows" % t
        assert_bits_equal(got["xyz"][t], out["xyz"].to_host()[0], "tile %d xyz" % t)
        assert_bits_equal(got["feat"][t], out["feat"].to_host()[0], "tile %d feat" % t)


# ---- 4. augment ---------------------------------------------------------------------------------------------------------------------------
def _augment_case():
    r = np.random.default_rng(21)
    xyz = ((r.random((4, N, 3), dtype=np.float32) - np.float32(0.5)) * np.array([30, 25, 8], np.float32)).astype(np.float32)
    theta = r.uniform(0, 2 * np.pi, 4)
    rot = np.stack([np.cos(theta), np.sin(theta)], axis=1)
    scale = r.uniform(0.8, 1.2, (4, 3))
    scale[1, 0] = -scale[1, 0]                                             # one negative x symmetry
    noise = r.normal(scale=0.001, size=(4, N, 3))
    return xyz, rot, scale, noise


def test_augment_restatement_against_the_reference_expression():
    xyz, rot, scale, noise = _augment_case()
    mine = FO.augment(xyz, rot, scale, noise)
    ref64 = np.stack([FO.augment_reference(xyz[t], rot[t], scale[t], noise[t]) for t in range(4)])
    ref = ref64.astype(np.float32)
    differ = int((mine.view(np.uint32) != ref.view(np.uint32)).sum())
    print("augment: %d of %d float32 values differ from the np.matmul form" % (differ, mine.size))
    ulp = np.abs(mine.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    same_sign = np.signbit(mine) == np.signbit(ref)
    assert (same_sign | ((mine == 0) & (ref == 0))).all() and ulp[same_sign].max() <= 1


def test_augment(backend):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    xyz, rot, scale, noise = _augment_case()
    rgb = np.random.default_rng(2).random((4, N, 3), dtype=np.float32)
    feat0 = np.concatenate([np.full((4, N, 3), 7, np.float32), rgb], axis=2)
    d_xyz, d_rot, d_scale, d_noise = DevArray.from_host(xyz), DevArray.from_host(rot), DevArray.from_host(scale), DevArray.from_host(noise)
    for with_noise in (True, False):
        d_feat = DevArray.from_host(feat0)
        _lib.check(_lib.lib().ssdr_feed_augment_dev(d_xyz.ptr, 4, N, d_rot.ptr, d_scale.ptr, d_noise.ptr if with_noise else None, 3, d_feat.ptr, None))
        _lib.sync()
        got = d_feat.to_host()
        assert_bits_equal(got[..., :3], FO.augment(xyz, rot, scale, noise if with_noise else None), "augmented xyz (noise: %s)" % with_noise)
        assert_bits_equal(got[..., 3:], rgb, "colour columns untouched")


# ---- 5. TrainFeeder -----------------------------------------------------------------------------------------------------------------------
def _cfg(dataset, batch, steps=3):
    from ssdr_al.helper_tool import ConfigS3DIS, ConfigSemantic3D

    class Small(ConfigS3DIS if dataset == "S3DIS" else ConfigSemantic3D):
        num_points = N
        num_layers = 5
        sub_sampling_ratio = [2, 2, 2, 2, 2]
        batch_size = batch
        train_steps = steps
    return Small


LEVELS = [1024, 512, 256, 128, 64, 32]


def _check_input_list(host, b):
    """the 26 arrays in the reference's order (s3dis_dataset.py:180-181), shapes and dtypes; pyramid and prefixes"""
    from ssdr_al import knn
    assert len(host) == 26
    for i in range(5):
        assert host[i].shape == (b, LEVELS[i], 3) and host[i].dtype == np.float32
        assert host[5 + i].shape == (b, LEVELS[i], 16) and host[5 + i].dtype == np.int32
        assert host[10 + i].shape == (b, LEVELS[i + 1], 16) and host[10 + i].dtype == np.int32
        assert host[15 + i].shape == (b, LEVELS[i], 1) and host[15 + i].dtype == np.int32
    for i, (w, dt) in enumerate([((N, 6), np.float32), ((N,), np.int32), ((N,), np.float32), ((N,), np.float32), ((N,), np.int32), ((), np.int32)]):
        assert host[20 + i].shape == (b,) + w and host[20 + i].dtype == dt, 20 + i
    neigh, sub, interp = knn.knn_pyramid(host[0], [2, 2, 2, 2, 2], 16)
    for i in range(5):
        assert np.array_equal(host[5 + i], neigh[i]), "neigh %d" % i
        assert np.array_equal(host[10 + i], neigh[i][:, : LEVELS[i + 1]]), "pool %d" % i
        assert np.array_equal(host[15 + i], interp[i]), "up %d" % i
        assert_bits_equal(host[i], host[0][:, : LEVELS[i]], "xyz level %d is the prefix" % i)


def _s3dis_feeder(seed=0, device_pair=False):
    from ssdr_al import training
    from ssdr_al._lib import DevArray
    clouds, _, _ = VO.make_case([300, 1024, 1029, 2117, 5000, 1500, 1100])
    acts, pses = _channels(clouds)
    if device_pair:
        pg = (DevArray.from_host(np.concatenate(acts)), DevArray.from_host(np.concatenate(pses)))
    else:
        pg = [np.stack([a, p]) for a, p in zip(acts, pses)]
    return training.TrainFeeder(clouds, pg, config=_cfg("S3DIS", 3, 10), dataset="S3DIS", seed=seed, color_scale=float(SCALE)), clouds, acts, pses, pg


def test_feeder_s3dis(backend):
    f, clouds, acts, pses, _ = _s3dis_feeder()
    assert f.one_epoch_steps == int(3 * 10 / 7 + 1) and f.steps_per_epoch == 3
    orders = []
    for epoch in range(2):
        seen, sizes = [], []
        for step, batch in enumerate(f.epoch_batches()):
            host = batch.to_host()
            # what a batch hands out is written by the generator alone: none of it is a buffer the upload stream writes (those are reused on `ready`,
            # before the consumer has run)
            uploaded = {st[k].ptr for st in f.sets for k in ("noise", "perm", "dup", "tile_cloud", "point")}
            assert not uploaded & ({a.ptr for a in batch.arrays} | {batch.center.ptr})
            d = f.draw(epoch, step)
            b = len(d["cloud"])
            sizes.append(b)
            if epoch == 0:
                _check_input_list(host, b)
            ref = FO.indep_batch(clouds, acts, pses, d["cloud"], d["point"], dict(d, dup=d["dup"]), N, SCALE)
            got = dict(zip(("feat", "labels", "act", "pse", "idx"), host[20:25]), xyz=host[0], center=batch.center.to_host())
            _compare(got, ref, "epoch %d batch %d" % (epoch, step))
            assert np.array_equal(host[25], d["cloud"])
            seen += host[25].tolist()
        assert sizes == [3, 3, 1] and sorted(seen) == list(range(7))       # every cloud once per epoch, the last batch partial
        orders.append(seen)
    assert orders[0] != orders[1]
    assert f.epoch == 2
    f.close()


def _sem3d_feeder(seed=3):
    from ssdr_al import training
    clouds, poss, _, weights, acts, pses = _weighted_case()
    pg = [np.stack([a, p]) for a, p in zip(acts, pses)]
    f = training.TrainFeeder(clouds, pg, config=_cfg("Semantic3D", 4, 3), dataset="Semantic3D", seed=seed, possibility=poss, color_scale=float(SCALE))
    return f, clouds, poss, weights, acts, pses, pg


def test_feeder_semantic3d(backend):
    from ssdr_al import training
    f, clouds, poss, weights, acts, pses, pg = _sem3d_feeder()
    assert np.array_equal(f.class_weight, weights)                         # the default: class frequencies over all labels
    gen = FO.ChainGenerator(clouds, poss, N, SCALE, xy_only=True, global_rows=False, class_weight=weights, activation=acts, pseudo=pses)
    for epoch in range(2):
        steps = 0
        for step, batch in enumerate(f.epoch_batches()):
            host = batch.to_host()
            uploaded = {st[k].ptr for st in f.sets for k in ("noise", "perm", "dup", "rot", "scale", "aug_noise")}
            assert not uploaded & ({a.ptr for a in batch.arrays} | {batch.center.ptr})
            d = f.draw(epoch, step)
            assert d["dup"] is None and d["aug_noise"].dtype == np.float64 and (np.abs(d["scale"][:, 0]) >= 0.8).all()
            ref = gen.batch(dict(d, dup=np.zeros((4, N), np.float32)))
            if epoch == 0 and step == 0:
                _check_input_list(host, 4)
            ref["feat"] = np.concatenate([FO.augment(ref["xyz"], d["rot"], d["scale"], d["aug_noise"]), ref["feat"][..., 3:]], axis=2)
            got = dict(zip(("feat", "labels", "act", "pse", "idx", "cloud"), host[20:26]), xyz=host[0], center=batch.center.to_host())
            assert np.array_equal(got["cloud"], ref["cloud"])
            _compare(got, ref, "epoch %d batch %d" % (epoch, step))
            steps += 1
        assert steps == 3                                                  # train_steps batches, then the epoch ends
        # the map carries into the next epoch
        assert np.array_equal(np.concatenate(f.possibility()), np.concatenate(gen.possibility)), "map after epoch %d" % epoch
    f.close()
    with pytest.raises(ValueError):                                        # a cloud below num_points: the reference's tree query would raise
        small, _, _ = VO.make_case([300, 1024])
        training.TrainFeeder(small, [np.zeros((2, 300), np.float32), np.zeros((2, 1024), np.float32)], config=_cfg("Semantic3D", 4, 3), dataset="Semantic3D")
    # labels index the weights: a class absent from the data makes the default table shorter than the label range, refused at construction
    gap = [dict(c, labels=np.where(c["labels"] == 2, 3, c["labels"])) for c in clouds]
    with pytest.raises(ValueError):
        training.TrainFeeder(gap, pg, config=_cfg("Semantic3D", 4, 3), dataset="Semantic3D")
    with pytest.raises(ValueError):
        training.TrainFeeder(clouds, pg, config=_cfg("Semantic3D", 4, 3), dataset="Semantic3D", class_weight=weights[:7])
    training.TrainFeeder(gap, pg, config=_cfg("Semantic3D", 4, 3), dataset="Semantic3D", class_weight=weights).close()


def test_feeder_device_pair_in_place_and_seeds(backend):
    from ssdr_al import _lib
    f, clouds, acts, pses, pair = _s3dis_feeder(seed=5, device_pair=True)
    assert f.d_act is pair[0] and f.d_pse is pair[1]                       # no copy
    g, _, _, _, _ = _s3dis_feeder(seed=5)
    b0, b1 = f.next_batch(), f.next_batch()                                # both buffer sets out: nothing further has been generated
    h0, h1 = b0.to_host(), b1.to_host()
    g0 = g.next_batch().to_host()
    for x, y in zip(h0, g0):                                               # equal seeds, equal batches (and the host list equals the device pair)
        assert_bits_equal(x, y, "equal seeds")
    cat_a = np.concatenate(acts)
    for h, step in ((h0, 0), (h1, 1)):
        rows = f.off[h[25]][:, None] + h[24]
        assert_bits_equal(h[22], cat_a[rows], "activation before the change")
    new_a = (cat_a + 2).astype(np.float32)
    _lib.check(_lib.lib().ssdr_memcpy_h2d(pair[0].ptr, _lib.ptr(new_a), new_a.nbytes))      # the next labelling writes the resident arrays
    b0.release(); b1.release()
    b2 = f.next_batch()
    h2 = b2.to_host()
    assert h2[22].shape == (1, N)
    assert_bits_equal(h2[22], new_a[f.off[h2[25]][:, None] + h2[24]], "activation after the change")
    b2.release()
    assert f.next_batch() is None
    f.close(); g.close()


@pytest.mark.parametrize("dataset", ["S3DIS", "Semantic3D"])
def test_equal_seeds_give_equal_epochs(backend, dataset):
    """two feeders with one seed: every array of every batch of two epochs (the partial batch, the augment draws), and the map; another seed differs"""
    mk = (lambda seed: _s3dis_feeder(seed=seed)[0]) if dataset == "S3DIS" else (lambda seed: _sem3d_feeder(seed=seed)[0])
    a, b, c = mk(9), mk(9), mk(10)
    differs = False
    for epoch in range(2):
        ha = [x.to_host() for x in a.epoch_batches()]
        hb = [x.to_host() for x in b.epoch_batches()]
        hc = [x.to_host() for x in c.epoch_batches()]
        assert len(ha) == len(hb) == len(hc) == 3
        for k, (x, y, z) in enumerate(zip(ha, hb, hc)):
            assert len(x) == len(y) == 26
            for i, (u, v) in enumerate(zip(x, y)):
                assert_bits_equal(u, v, "epoch %d batch %d array %d" % (epoch, k, i))
            differs |= not np.array_equal(x[20], z[20])
    assert differs
    if dataset == "Semantic3D":
        assert np.array_equal(np.concatenate(a.possibility()), np.concatenate(b.possibility()))
    for f in (a, b, c):
        f.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    L = _lib.lib()
    clouds, poss, rng = VO.make_case([300, 1024])
    acts, pses = _channels(clouds)
    dev = _Dev(clouds, acts, pses, poss)
    before = dev.state()
    B = 2
    d = VO.draw_batch(rng, np.random.default_rng(1), B, N)
    d_n, d_perm, d_dup = DevArray.from_host(d["noise"]), DevArray.from_host(d["perm"]), DevArray.from_host(d["dup"])
    o = _Dev.outputs(B)
    d_w = DevArray.from_host(np.full(13, 0.5))
    d_tc, d_tp = DevArray.from_host(np.array([0, 1], np.int32)), DevArray.from_host(np.array([5, 7], np.int32))

    def chain(off=dev.off, nc=2, tiles=B, points=N, pts=True, labels=True, out_labels=True, weights=False, act_in=True, act_out=True):
        off = np.ascontiguousarray(off, np.int64)
        return L.ssdr_feed_chain_dev(dev.d_p.ptr if pts else None, dev.d_c.ptr, 3, dev.d_l.ptr if labels else None, dev.d_poss.ptr, dev.d_min.ptr, dev.d_arg.ptr, _lib.ptr(off), nc,
                                     tiles, points, d_n.ptr, d_perm.ptr, d_dup.ptr, 1.0, o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr, o["labels"].ptr if out_labels else None,
                                     o["cloud"].ptr, o["center"].ptr, XY_ONLY, d_w.ptr if weights else None, 13 if weights else 0,
                                     dev.d_a.ptr if act_in else None, dev.d_s.ptr, o["act"].ptr if act_out else None, o["pse"].ptr, None)

    def tiles(off=dev.off, nc=2, n_tiles=B, points=N, tc=True, pse_in=True):
        off = np.ascontiguousarray(off, np.int64)
        return L.ssdr_feed_tiles_dev(dev.d_p.ptr, dev.d_c.ptr, 3, dev.d_l.ptr, dev.d_a.ptr, dev.d_s.ptr if pse_in else None, _lib.ptr(off), nc, n_tiles, points,
                                     d_tc.ptr if tc else None, d_tp.ptr, d_n.ptr, d_perm.ptr, d_dup.ptr, 1.0, o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr, o["labels"].ptr,
                                     o["act"].ptr, o["pse"].ptr, o["cloud"].ptr, o["center"].ptr, None)

    many = np.arange(4098, dtype=np.int64)
    assert chain(pts=False) == SSDR_ERR_INVALID and tiles(tc=False) == SSDR_ERR_INVALID                      # null arguments
    assert chain(nc=0) == SSDR_ERR_INVALID and tiles(nc=0) == SSDR_ERR_INVALID                               # no clouds
    assert chain([0, 300, 300]) == SSDR_ERR_INVALID and tiles([0, 300, 300]) == SSDR_ERR_INVALID             # an empty cloud
    assert chain(many, 4097) == SSDR_ERR_UNSUPPORTED and tiles(many, 4097) == SSDR_ERR_UNSUPPORTED           # 4 097 clouds
    assert chain([0, 300, 0x40000000]) == SSDR_ERR_UNSUPPORTED and tiles([0, 300, 0x40000000]) == SSDR_ERR_UNSUPPORTED
    assert chain(tiles=0) == SSDR_ERR_INVALID and tiles(n_tiles=0) == SSDR_ERR_INVALID                       # zero tiles
    # every NULL is refused before any size, as ssdr_vote_tiles_dev has always ordered it: NULL map and too many rows -> INVALID, not UNSUPPORTED
    off2 = np.ascontiguousarray(dev.off, np.int64)
    head = lambda poss_ptr: (dev.d_p.ptr, dev.d_c.ptr, 3, dev.d_l.ptr, poss_ptr, dev.d_min.ptr, dev.d_arg.ptr, _lib.ptr(off2), 2, 2, 0x3fffffff, d_n.ptr, d_perm.ptr, d_dup.ptr,
                              1.0, o["xyz"].ptr, o["feat"].ptr, o["idx"].ptr, o["labels"].ptr, o["cloud"].ptr, o["center"].ptr)
    assert L.ssdr_vote_tiles_dev(*head(None), None) == SSDR_ERR_INVALID and L.ssdr_vote_tiles_dev(*head(dev.d_poss.ptr), None) == SSDR_ERR_UNSUPPORTED
    assert L.ssdr_feed_chain_dev(*head(None), 0, None, 0, None, None, None, None, None) == SSDR_ERR_INVALID
    assert tiles(tc=False, points=0x3fffffff) == SSDR_ERR_INVALID and tiles(points=0x3fffffff) == SSDR_ERR_UNSUPPORTED
    assert chain(points=0) == SSDR_ERR_INVALID and tiles(points=0) == SSDR_ERR_INVALID
    assert chain(labels=False) == SSDR_ERR_INVALID                                                           # labels wanted but missing
    assert chain(labels=False, out_labels=False, weights=True) == SSDR_ERR_INVALID                           # weights without labels
    assert chain(act_in=False) == SSDR_ERR_INVALID and tiles(pse_in=False) == SSDR_ERR_INVALID               # a channel output without its input
    assert L.ssdr_feed_augment_dev(None, 2, N, d_n.ptr, d_n.ptr, None, 3, o["feat"].ptr, None) == SSDR_ERR_INVALID
    assert L.ssdr_feed_augment_dev(o["xyz"].ptr, 0, N, d_n.ptr, d_n.ptr, None, 3, o["feat"].ptr, None) == SSDR_ERR_INVALID
    _lib.sync()
    after = dev.state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))                                          # nothing was launched
    status = np.zeros(1, np.int32)
    assert L.ssdr_feed_status(None, _lib.ptr(status)) == 0 and status[0] == 0
    assert chain(act_in=False, act_out=False) == 0 and chain(weights=True) == 0                              # ... and these run
    # a tile's cloud or point out of range: a zero tile and a status bit, the other tile as ever
    good = dev.tiles([0, 1], [5, 7], d)
    assert L.ssdr_feed_status(None, _lib.ptr(status)) == 0 and status[0] == 0
    for tc, tp, bit in (([0, 2], [5, 7], 2), ([0, -1], [5, 7], 2), ([0, 1], [5, 1024], 4), ([0, 1], [5, -3], 4)):
        got = dev.tiles(tc, tp, d)
        assert L.ssdr_feed_status(None, _lib.ptr(status)) == SSDR_ERR_INVALID and status[0] == bit, (tc, tp)
        for k, v in got.items():
            assert not v[1].any(), k                                                                          # the zero tile
            assert np.array_equal(v[0].view(np.uint32) if v.dtype == np.float32 else v[0], good[k][0].view(np.uint32) if v.dtype == np.float32 else good[k][0]), k


@pytest.mark.gpu
def test_generators_at_the_workload_tile_size():
    """num_points 40 960 over clouds of 90 000, 30 000 (smaller than a tile) and 150 000 points: 6 independent tiles, then 8 tiles of the weighted chain"""
    from conftest import GPU_LIB, _have_gpu
    from ssdr_al import _lib
    if not _have_gpu():
        pytest.skip("no GPU")
    _lib.use(GPU_LIB)
    big = 40960
    try:
        clouds, poss, rng = VO.make_case([90000, 30000, 150000])
        r = np.random.default_rng(11)
        for c in clouds:
            c["labels"] = r.integers(0, 8, len(c["xyz"])).astype(np.int32)
        clouds[2]["labels"][:100000] = 4
        _, cnt = np.unique(np.concatenate([c["labels"] for c in clouds]), return_counts=True)
        weights = cnt / np.sum(cnt)
        acts, pses = _channels(clouds)
        dev = _Dev(clouds, acts, pses, poss, num_points=big)
        tile_cloud = np.array([2, 0, 1, 2, 0, 1], np.int32)
        tile_point = np.array([rng.integers(0, len(clouds[c]["xyz"])) for c in tile_cloud], np.int32)
        d = VO.draw_batch(rng, np.random.default_rng(99), 6, big)
        _compare(dev.tiles(tile_cloud, tile_point, d), FO.indep_batch(clouds, acts, pses, tile_cloud, tile_point, d, big, SCALE), "tiles")
        d = VO.draw_batch(rng, np.random.default_rng(98), 8, big)
        gen = FO.ChainGenerator(clouds, poss, big, SCALE, xy_only=True, global_rows=False, class_weight=weights, activation=acts, pseudo=pses)
        ref = gen.batch(d)
        got = dev.chain(d, XY_ONLY, weights)
        assert np.array_equal(got["cloud"], ref["cloud"]) and len(set(ref["cloud"].tolist())) == 3
        _compare(got, ref, "chain")
        st = dev.state()
        assert np.array_equal(st[0], np.concatenate(gen.possibility)) and np.array_equal(st[1], gen.min_possibility) and np.array_equal(st[2], gen.cloud_arg())
    finally:
        _lib.use(None)
