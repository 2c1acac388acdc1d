"""The generators' per-row draws made on the device (ssdr_draw_perm_dev / ssdr_draw_uniform_dev / ssdr_draw_normal_dev, ssdr_al.draws, and
draws="device" of VoteTester and TrainFeeder) against the NumPy restatement of the counter chain (tests/_draw_oracle.py), and, for what must not
rest on a restatement its author also wrote, against properties: every row a permutation, every counter word changes the row, chi-square
uniformity at the bar NumPy's own generator is held to first.

Every test asserts its input condition before it compares anything."""
import ctypes as C
import math

import numpy as np
import pytest

import _draw_oracle as O
import _vote_oracle as VO
from conftest import assert_bits_equal

SSDR_ERR_INVALID, SSDR_ERR_UNSUPPORTED = 1, 5
RADIX_TILE = 2048
SEED, EPOCH, STEP = 0x1234567887654321, 3, 11


def _draws():
    from ssdr_al import _lib, draws
    _lib.check(_lib.lib().ssdr_init(0))
    return draws


def _stream():
    from ssdr_al import _lib
    p = C.c_void_p()
    _lib.check(_lib.lib().ssdr_stream_create(C.byref(p)))
    return p.value


def _drop(stream):
    from ssdr_al import _lib
    _lib.sync(stream)
    _lib.lib().ssdr_stream_destroy(stream)


# ---- 1. permutations, index for index against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (1, 2), (3, 2047), (2, 2048), (3, 2049), (5, 4097), (20, 40960), (4, 65536), (2, 1024), (3, 1025), (70, 1025), (300, 7)])
def test_perm_matches_restatement(backend, B, N):
    """the sort tile's edges, the workloads' own shapes, and the layout's: 1024 rows are the largest tiles that share a segment, 1025 the smallest
    that own one, 70 such tiles are more segments than one round of the sort takes (64), 300 tiles of 7 rows share two sort tiles"""
    D = _draws()
    keys = O.perm_keys(SEED, EPOCH, STEP, 0, B, N)
    assert keys.shape == (B, N) and int(keys.max()) < 1 << 32
    if N > 1:
        assert len(np.unique(keys)) > 1                                    # the keys do order something
    got = D.perm(SEED, EPOCH, STEP, B, N).to_host()
    assert got.dtype == np.int32 and got.shape == (B, N)
    assert np.array_equal(got, O.perm(SEED, EPOCH, STEP, B, N))


def test_perm_ties_come_out_in_index_order(backend):
    D = _draws()
    B, N, bits = 3, 5000, 4
    keys = O.perm_keys(SEED, EPOCH, STEP, 0, B, N, key_bits=bits)
    for t in range(B):
        assert np.bincount(keys[t].astype(np.int64), minlength=16).min() > 1          # all 16 key values, each more than once: ties everywhere
    got = D.perm(SEED, EPOCH, STEP, B, N, key_bits=bits).to_host()
    assert np.array_equal(got, O.perm(SEED, EPOCH, STEP, B, N, key_bits=bits))
    for t in range(B):                                                     # and said without the argsort: inside a run of equal keys the rows ascend
        k = keys[t][got[t]]
        assert (np.diff(k.astype(np.int64)) >= 0).all()
        same = np.diff(k.astype(np.int64)) == 0
        assert (np.diff(got[t])[same] > 0).all()


@pytest.mark.parametrize("N", [64, 4097])
def test_perm_first_tile_is_a_slice(backend, N):
    D = _draws()
    whole = D.perm(SEED, EPOCH, STEP, 5, N).to_host()
    part = D.perm(SEED, EPOCH, STEP, 3, N, first_tile=2).to_host()
    assert not np.array_equal(whole[:3], whole[2:5])
    assert np.array_equal(part, whole[2:5])
    assert np.array_equal(part, O.perm(SEED, EPOCH, STEP, 3, N, first_tile=2))


def test_perm_scratch_regrowth_and_streams(backend):
    """large, small, large on one (caller's) stream: the scratch grows once and is reused; two streams interleaved: each has its own"""
    from ssdr_al import _lib
    D = _draws()
    s1, s2 = _stream(), _stream()
    assert s1 != s2
    shapes = [(6, 9000), (2, 100), (7, 9000), (3, 3000)]
    assert shapes[0][0] * shapes[0][1] < shapes[2][0] * shapes[2][1] and shapes[1][0] * shapes[1][1] < RADIX_TILE
    outs = [D.perm(SEED, EPOCH, i, B, N, stream=s1) for i, (B, N) in enumerate(shapes)]
    _lib.sync(s1)
    for i, ((B, N), o) in enumerate(zip(shapes, outs)):
        assert np.array_equal(o.to_host(s1), O.perm(SEED, EPOCH, i, B, N)), (B, N)
    a, b = [], []
    for i in range(3):                                                     # nothing waits in between: a shared scratch would be overwritten
        a.append(D.perm(SEED, 1, i, 4, 5000 + i, stream=s1))
        b.append(D.perm(SEED, 2, i, 9, 2500 + i, stream=s2))
    _lib.sync(s1); _lib.sync(s2)
    for i in range(3):
        assert np.array_equal(a[i].to_host(s1), O.perm(SEED, 1, i, 4, 5000 + i))
        assert np.array_equal(b[i].to_host(s2), O.perm(SEED, 2, i, 9, 2500 + i))
    _drop(s1); _drop(s2)


def test_refusals(backend):
    from ssdr_al import _lib
    from ssdr_al._lib import DevArray
    D = _draws()
    L = D._bind(_lib.lib())
    d = DevArray.from_host(np.full(16, -7, np.int32))
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 2, 8, 32, None, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 0, 8, 32, d.ptr, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 2, 0, 32, d.ptr, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 2, 8, 0, d.ptr, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 2, 8, 33, d.ptr, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_perm_dev(1, 0, 0, (1 << 32) - 1, 2, 8, 32, d.ptr, None) == SSDR_ERR_INVALID          # a tile id of 2^32
    # 2^19 tiles of 2049 rows own 4096 slots each: 2^31 padded pairs, although the dense array would have had fewer than 0x3fffffff * 2
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 1 << 19, 2049, 32, d.ptr, None) == SSDR_ERR_UNSUPPORTED
    assert L.ssdr_draw_perm_dev(1, 0, 0, 0, 1, 1 << 30, 32, d.ptr, None) == SSDR_ERR_UNSUPPORTED
    assert "0x3fffffff" in _lib.lib().ssdr_last_error().decode()
    f = DevArray.from_host(np.full(16, -7, np.float32)); g = DevArray.from_host(np.full(16, -7, np.float64))
    assert L.ssdr_draw_uniform_dev(1, 0, 0, 1, 0, 16, None, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_uniform_dev(1, 0, 0, 1, 0, 0, f.ptr, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_normal_dev(1, 0, 0, 2, 0, 16, 1.0, None, None) == SSDR_ERR_INVALID
    assert L.ssdr_draw_normal_dev(1, 0, 0, 2, 0, 0, 1.0, g.ptr, None) == SSDR_ERR_INVALID
    _lib.sync()
    assert (d.to_host() == -7).all() and (f.to_host() == -7).all() and (g.to_host() == -7).all()             # refused before any launch
    # and the last legal tile id works
    assert L.ssdr_draw_perm_dev(1, 0, 0, (1 << 32) - 1, 1, 16, 32, d.ptr, None) == 0
    _lib.sync()
    assert np.array_equal(d.to_host(), O.perm(1, 0, 0, 1, 16, first_tile=(1 << 32) - 1)[0])


# ---- 2. permutations, without the restatement ----------------------------------------------------------------------------------------------------
def test_every_row_is_a_permutation_and_every_counter_word_counts(backend):
    D = _draws()
    for B, N in [(7, 1), (9, 64), (5, 2049), (3, 40960)]:
        p = D.perm(SEED, EPOCH, STEP, B, N).to_host()
        assert np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(N, dtype=np.int32), (B, N))), (B, N)
    N = 512
    base = D.perm(SEED, EPOCH, STEP, 4, N).to_host()
    others = dict(seed_low=D.perm(SEED ^ 1, EPOCH, STEP, 4, N), seed_high=D.perm(SEED ^ (1 << 63), EPOCH, STEP, 4, N), epoch=D.perm(SEED, EPOCH + 1, STEP, 4, N),
                  step=D.perm(SEED, EPOCH, STEP + 1, 4, N), epoch_step_swapped=D.perm(SEED, STEP, EPOCH, 4, N))
    for what, o in others.items():
        o = o.to_host()
        for t in range(4):
            assert not np.array_equal(o[t], base[t]), what
    for t in range(4):                                                     # the tile: no two rows of a call agree
        for u in range(t):
            assert not np.array_equal(base[t], base[u])


def _chi2_bar(df=63, q=1e-6):
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - q, df))
    except ImportError:                                                    # Wilson-Hilferty; z = the 1 - 1e-6 quantile of the standard normal
        z = 4.753424308822899
        return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


def _uniformity(p):
    """chi-square statistics (63 degrees of freedom each) of T permutations of N = 64: the value at row 0; membership in the first N / 4 rows (what
    random_sample keeps), whose counts are binomial(T, 1/4): variance factor 3/4"""
    T, N = p.shape
    first = np.bincount(p[:, 0], minlength=N).astype(np.float64)
    kept = np.bincount(p[:, : N // 4].ravel(), minlength=N).astype(np.float64)
    return float(((first - T / N) ** 2 / (T / N)).sum()), float(((kept - T / 4) ** 2 / (T / 4 * 0.75)).sum())


@pytest.mark.parametrize("seed", [1, 2, 3, 5, 8, 13, 21, 34])
def test_perm_uniformity(backend, seed):
    D = _draws()
    T, N = 8192, 64
    bar = _chi2_bar()
    assert abs(bar - 131.4) < 0.1
    rng = np.random.default_rng(seed)
    ref = _uniformity(np.stack([rng.permutation(N) for _ in range(T)]))
    print("seed %d: NumPy's generator %.1f %.1f" % ((seed,) + ref))
    assert max(ref) < bar                                                  # the bar holds NumPy's own generator first
    got = _uniformity(D.perm(seed, 0, 0, T, N).to_host())
    print("seed %d: device draws      %.1f %.1f" % ((seed,) + got))
    assert max(got) < bar


# ---- 3. uniform --------------------------------------------------------------------------------------------------------------------------------
def test_uniform(backend):
    D = _draws()
    n, avail = 1 << 20, 65535
    ref = O.uniform(SEED, EPOCH, STEP, O.DUP, n)
    assert ref.dtype == np.float32 and ref.max() >= 1 - 2.0 ** -16 and ref.min() < 2.0 ** -16           # both ends of the range are reached
    got = D.uniform(SEED, EPOCH, STEP, D.DUP, n).to_host()
    assert_bits_equal(got, ref, "uniform")
    assert got.max() < 1 and got.min() >= 0
    pick = np.floor(got * np.float32(avail))                               # data_aug's padding pick, in float32 as the generator forms it
    assert pick.dtype == np.float32 and pick.max() < avail and pick.max() == avail - 1
    for first, m in [(1, 1), (255, 258), (n - 1000, 1000)]:                # slices through `first`, across a block's edge
        assert_bits_equal(D.uniform(SEED, EPOCH, STEP, D.DUP, m, first=first).to_host(), ref[first:first + m], "slice at %d" % first)
    beyond = D.uniform(SEED, EPOCH, STEP, D.DUP, 8, first=(1 << 32) - 4).to_host()                       # the element's high word
    assert_bits_equal(beyond, O.uniform(SEED, EPOCH, STEP, O.DUP, 8, first=(1 << 32) - 4), "across 2^32")
    assert not np.array_equal(beyond[4:], ref[:4])
    other = D.uniform(SEED, EPOCH, STEP, D.AUG_NOISE, 64).to_host()
    assert not np.array_equal(other, ref[:64])                             # the kind is part of the counter


# ---- 4. normal ---------------------------------------------------------------------------------------------------------------------------------
def _ks_p(x):
    try:
        from scipy.stats import kstest
        return float(kstest(x, "norm").pvalue)
    except ImportError:                                                    # Kolmogorov's asymptotic series
        n = len(x)
        cdf = 0.5 * (1 + np.frompyfunc(math.erf, 1, 1)(np.sort(x) / math.sqrt(2)).astype(np.float64))
        d = max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max())
        return float(min(1.0, 2 * sum((-1) ** (k - 1) * math.exp(-2 * k * k * n * d * d) for k in range(1, 101))))


def _normal_bars(x, what):
    n = len(x)
    mean, var, p = float(x.mean()), float(x.var()), _ks_p(x)
    print("%s: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e), KS p %.3g" % (what, mean, 6 / math.sqrt(n), var - 1, 6 * math.sqrt(2 / n), p))
    assert abs(mean) <= 6 / math.sqrt(n) and abs(var - 1) <= 6 * math.sqrt(2 / n) and p > 1e-6, what


def test_normal(backend):
    """|dev - np| <= 1e-12 * scale: R = sqrt(-2 ln u1) <= 8.6 for u1 >= 2^-53; a few ulp on each of log, sqrt, cos and the products on either side
    come to about 2e-14; the bar is 50 times that.  Measured at scale 1 over 2^20 values: 4.4e-16 on the CPU logic build, 6.7e-16 on gfx950."""
    D = _draws()
    n = 1 << 20
    for scale in (1.0, 0.001):
        ref = O.normal(SEED, EPOCH, STEP, O.AUG_NOISE, n, scale=scale)
        assert ref.dtype == np.float64 and np.isfinite(ref).all() and np.abs(ref).max() > 4 * scale      # the tails are there
        got = D.normal(SEED, EPOCH, STEP, D.AUG_NOISE, n, scale=scale).to_host()
        diff = float(np.abs(got - ref).max())
        print("normal, scale %g: largest difference to the restatement %.3e (%s build)" % (scale, diff, backend))
        assert diff <= 1e-12 * scale
    for first, m in [(3, 1), (250, 520), (n - 7, 7)]:                      # slices through `first`: the same bits as the whole call
        assert np.array_equal(D.normal(SEED, EPOCH, STEP, D.AUG_NOISE, m, scale=0.001, first=first).to_host(), got[first:first + m])
    _normal_bars(np.random.default_rng(4).normal(size=n), "NumPy's generator")       # the bars hold NumPy's own generator first
    _normal_bars(D.normal(SEED, EPOCH, STEP, D.AUG_NOISE, n).to_host(), "device draws")


# ---- 5. the feeders ------------------------------------------------------------------------------------------------------------------------------
N = 1024
SIZES = [300, 1024, 1029, 2117, 5000]


def _restated(feeder, with_noise):
    """a host-mode draws= callable: the device-mode feeder's own per-tile draws plus the restated per-row draws"""
    def draws(epoch, step):
        d = dict(feeder.draw(epoch, step))
        b = len(d["noise"])
        assert not {"perm", "dup", "aug_noise"} & set(d)                   # nothing per row comes from the host in device mode
        d["perm"] = O.perm(feeder.seed, epoch, step, b, N)
        d["dup"] = O.uniform(feeder.seed, epoch, step, O.DUP, b * N).reshape(b, N)
        if with_noise:
            d["aug_noise"] = O.normal(feeder.seed, epoch, step, O.AUG_NOISE, b * N * 3, scale=feeder.augment_noise).reshape(b, N, 3)
        return d
    return draws


def test_vote_tester_device_draws(backend):
    from oracle import randla_np as R
    from ssdr_al import evaluate
    from ssdr_al.helper_tool import ConfigS3DIS

    class Small(ConfigS3DIS):
        num_points = N
        num_layers = 2
        d_out = [16, 64]
        sub_sampling_ratio = [4, 4]
        num_classes = 13
        val_batch_size = 8
        val_steps = 1
        noise_init = 3.5
    weights = R.init_weights(0, d_out=(16, 64))
    with pytest.raises(ValueError):
        evaluate.VoteTester(weights, [], config=Small, draws="bogus")
    clouds, poss, _ = VO.make_case(SIZES)
    poss = VO.add_ties(poss)
    dev = evaluate.VoteTester(weights, clouds, config=Small, possibility=poss, seed=21, draws="device")
    host = evaluate.VoteTester(weights, clouds, config=Small, possibility=poss, seed=21)
    assert dev.pads and dev.draws == "device" and host.draws == "host"
    assert set(dev.draw(0, 0)) == {"noise"} and set(host.draw(0, 0)) == {"noise", "perm", "dup"}
    restated = _restated(dev, False)
    padded = 0
    for epoch in range(2):
        assert dev.evaluate(max_epochs=1) == (0, 0) and host.evaluate(max_epochs=1, draws=restated) == (0, 0)
        a, b = dev.sets[epoch % dev.DEPTH], host.sets[epoch % host.DEPTH]
        cloud = a["cloud"].to_host(dev.s_gen)
        padded += int((cloud == 0).sum())
        assert np.array_equal(cloud, b["cloud"].to_host(host.s_gen))
        for k in ("idx", "labels"):
            assert np.array_equal(a[k].to_host(dev.s_gen), b[k].to_host(host.s_gen)), k
        for k in ("xyz", "feat", "center"):
            assert_bits_equal(a[k].to_host(dev.s_gen), b[k].to_host(host.s_gen), "epoch %d %s" % (epoch, k))
        assert np.array_equal(a["perm"].to_host(dev.s_gen), O.perm(21, epoch, 0, 8, N))
        assert np.array_equal(np.concatenate(dev.possibility()), np.concatenate(host.possibility()))
        for x, y in zip(dev.cloud_state(), host.cloud_state()):
            assert np.array_equal(x, y)
    assert padded > 0                                                      # the 300-point cloud was cut: the padding draws decided rows
    assert dev.epochs == 2 and dev.tiles == 16 and dev.min_history == host.min_history
    probs = dev.probs_host()
    assert np.abs(probs).max() > 0
    assert_bits_equal(probs, host.probs_host(), "test_probs")
    # the rule is per key: a callable that does return a permutation has it uploaded, the padding draws still come from the device
    mixed = evaluate.VoteTester(weights, clouds, config=Small, possibility=poss, seed=21, draws="device")
    mixed.evaluate(max_epochs=1, draws=lambda e, s: dict(dev.draw(e, s), perm=O.perm(21, e, s, 8, N)))
    assert np.array_equal(mixed.sets[0]["idx"].to_host(mixed.s_gen), dev.sets[0]["idx"].to_host(dev.s_gen))          # epoch 0's batch again
    assert_bits_equal(mixed.sets[0]["xyz"].to_host(mixed.s_gen), dev.sets[0]["xyz"].to_host(dev.s_gen), "mixed xyz")
    with pytest.raises(KeyError):                                          # host mode: a per-row key that is absent is an error, as before
        host.run_batch(dev.draw(0, 0))
    for x in (dev, host, mixed):
        x.close()


def _cfg(dataset, batch, steps=3):
    from ssdr_al.helper_tool import ConfigS3DIS, ConfigSemantic3D

    class Small(ConfigS3DIS if dataset == "S3DIS" else ConfigSemantic3D):
        num_points = N
        num_layers = 5
        sub_sampling_ratio = [2, 2, 2, 2, 2]
        batch_size = batch
        train_steps = steps
    return Small


def _channels(clouds, seed=5):
    r = np.random.default_rng(seed)
    return ([(r.random(len(c["xyz"])) < 0.3).astype(np.float32) for c in clouds], [r.integers(0, 8, len(c["xyz"])).astype(np.float32) for c in clouds])


def _feeder(dataset, seed, draws):
    from ssdr_al import training
    if dataset == "S3DIS":
        clouds, _, _ = VO.make_case([300, 1024, 1029, 2117, 5000, 1500, 1100])
        poss = None
    else:
        clouds, poss, _ = VO.make_case([1024, 1029, 2117, 5000])
        r = np.random.default_rng(11)
        for c in clouds:
            c["labels"] = r.integers(0, 8, len(c["xyz"])).astype(np.int32)
    acts, pses = _channels(clouds)
    pg = [np.stack([a, p]) for a, p in zip(acts, pses)]
    return training.TrainFeeder(clouds, pg, config=_cfg(dataset, 3 if dataset == "S3DIS" else 4, 10 if dataset == "S3DIS" else 3), dataset=dataset, seed=seed,
                                possibility=poss, color_scale=1.0 / 255.0, draws=draws)


def _epochs(feeder, draws=None, epochs=2):
    out = []
    for _ in range(epochs):
        out.append([(b.to_host(), b.center.to_host(feeder.s_gen)) for b in feeder.epoch_batches(draws=draws)])
    return out


def _ordered(a):
    """float32 bits as integers that ascend with the value: a difference of 1 is one ulp"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def test_train_feeder_s3dis_device_draws(backend):
    from ssdr_al import training
    with pytest.raises(ValueError):
        _feeder("S3DIS", 0, "bogus")
    dev, host = _feeder("S3DIS", 6, "device"), _feeder("S3DIS", 6, "host")
    assert dev.pads and isinstance(dev, training.TrainFeeder)
    assert set(dev.draw(0, 0)) == {"noise", "cloud", "point"} and {"perm", "dup"} <= set(host.draw(0, 0))
    got, ref = _epochs(dev), _epochs(host, _restated(dev, False))
    sizes, seen = [], []
    for epoch in range(2):
        assert len(got[epoch]) == len(ref[epoch]) == 3
        for k, ((x, cx), (y, cy)) in enumerate(zip(got[epoch], ref[epoch])):
            assert len(x) == len(y) == 26
            for i, (u, v) in enumerate(zip(x, y)):
                assert_bits_equal(u, v, "epoch %d batch %d array %d" % (epoch, k, i))
            assert_bits_equal(cx, cy, "centres")
            sizes.append(len(x[25])); seen += x[25].tolist()
    assert sizes == [3, 3, 1] * 2 and 0 in seen                            # the partial batch, and the 300-point cloud: padded through the device's draws
    dev.close(); host.close()


def test_train_feeder_semantic3d_device_draws(backend):
    dev, host = _feeder("Semantic3D", 4, "device"), _feeder("Semantic3D", 4, "host")
    assert dev.augment_noise == 0.001 and not dev.pads
    assert set(dev.draw(0, 0)) == {"noise", "rot", "scale"} and "aug_noise" in host.draw(0, 0)
    got, ref = _epochs(dev), _epochs(host, _restated(dev, True))
    differ = total = 0
    for epoch in range(2):
        assert len(got[epoch]) == len(ref[epoch]) == 3
        for k, ((x, cx), (y, cy)) in enumerate(zip(got[epoch], ref[epoch])):
            for i, (u, v) in enumerate(zip(x, y)):
                if i == 20:                                                # features: the three augmented columns may differ by one float32 ulp
                    assert_bits_equal(u[..., 3:], v[..., 3:], "colour columns")
                    ulp = np.abs(_ordered(u[..., :3]) - _ordered(v[..., :3]))
                    assert ulp.max() <= 1
                    differ += int((ulp != 0).sum()); total += ulp.size
                else:
                    assert_bits_equal(u, v, "epoch %d batch %d array %d" % (epoch, k, i))
            assert_bits_equal(cx, cy, "centres")
    print("augmented feature elements that differ by one ulp: %d of %d" % (differ, total))
    assert differ <= 1e-4 * total
    assert np.array_equal(np.concatenate(dev.possibility()), np.concatenate(host.possibility()))
    dev.close(); host.close()


@pytest.mark.parametrize("dataset", ["S3DIS", "Semantic3D"])
def test_equal_seeds_give_equal_epochs_in_device_mode(backend, dataset):
    a, b, c = _feeder(dataset, 9, "device"), _feeder(dataset, 9, "device"), _feeder(dataset, 10, "device")
    ha, hb, hc = _epochs(a), _epochs(b), _epochs(c)
    differs = False
    for epoch in range(2):
        assert len(ha[epoch]) == 3
        for (x, _), (y, _), (z, _) in zip(ha[epoch], hb[epoch], hc[epoch]):
            for i, (u, v) in enumerate(zip(x, y)):
                assert_bits_equal(u, v, "epoch %d array %d" % (epoch, i))
            differs |= not np.array_equal(x[24], z[24])
    assert differs                                                         # another seed: other rows
    if dataset == "Semantic3D":
        assert np.array_equal(np.concatenate(a.possibility()), np.concatenate(b.possibility()))
    for f in (a, b, c):
        f.close()
