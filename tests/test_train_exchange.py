"""Trainer(comm=): the data-parallel training step (csrc/train_exchange.hip, DESIGN section 21 "Data-parallel") equals the single-process step over
the union of all ranks' tiles.

1. the merges alone against a NumPy float32 restatement of the same operations in the same order, bit for bit (CPU logic build and gfx950);
2. world 1 through the exchange (gloo / RCCL in a child) is the plain trainer, every bit;
3. worlds 2 (2 + 1 tiles) and 3 (1 + 1 + 1) over gloo against the float64 oracle over the union, bars of tests/test_randla_train.py with the
   UNION's reduction rows;
4. edges: a rank without a valid row, no valid row anywhere, a callback that raises, unequal batch counts, no exchange in inference mode, refusals;
5. the symbols in both libraries;   6. the pieces under ASan + UBSan in a stand-alone program.
The worker of the children is tests/_train_dist_worker.py.

invstd = 1 / sqrt(var + eps) is bit-equal to NumPy's on both builds (measured: 0 ulp on the CPU logic build and on one MI355X; the gfx950 build
divides and takes square roots correctly rounded by default), so the 2 ulp fall-back the GPU is allowed is not in use."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _train_cases as TC
import _train_dist_worker as WK
from conftest import ROOT, assert_bits_equal

U = 2.0 ** -24
MIN_VAR = 1e-3
SSDR_ERR_INVALID = 1
F = np.float32
WORKER = os.path.join(ROOT, "tests", "_train_dist_worker.py")
SYMBOLS = ("ssdr_randla_train_set_exchange", "ssdr_randla_train_exchange", "ssdr_bn_stats_merge_dev", "ssdr_rank_sums_merge_dev",
           "ssdr_randla_train_dropout_mask_range_dev")


def _lib_bound():
    from ssdr_al import _lib, trainer
    return _lib, trainer._bind(_lib.lib())


def _dev(a):
    from ssdr_al._lib import DevArray
    return DevArray.from_host(np.ascontiguousarray(a))


# ---- 1. the merges alone ----------------------------------------------------------------------------------------------------------------------
COUNTS = {1: [517], 2: [1, 3932160], 3: [3, 1, 3932160], 8: [3, 1, 3932160, 517, 40960, 2, 64, 100000]}      # 3 932 160 = 6 x 40 960 x 16 rows


def _records(world, Cn, seed):
    """[world][1 + 2C]: unequal row counts; the even channels' means are ~1e3 with a spread of ~1e-2 between the ranks (and a variance to match),
    the odd ones of order 1; a rank with one row has M2 = 0"""
    rng = np.random.default_rng([seed, world, Cn])
    rec = np.zeros((world, 1 + 2 * Cn), F)
    big = (np.arange(Cn) % 2 == 0)
    centre = np.where(big, 1000.0 + rng.normal(0, 20, Cn), rng.normal(0, 1, Cn))
    for r, n in enumerate(COUNTS[world]):
        rec[r, 0] = n
        rec[r, 1:1 + Cn] = centre + np.where(big, 1e-2, 0.3) * rng.normal(0, 1, Cn)
        var = np.where(big, 1e-4, 1.0) * rng.uniform(0.05, 0.5, Cn)
        rec[r, 1 + Cn:] = 0.0 if n == 1 else n * var
    return rec


def bn_merge_np(rec, mov_mean, mov_var, unbiased):
    """merge_stats_kernel, operation for operation, in float32"""
    world, Cn = rec.shape[0], (rec.shape[1] - 1) // 2
    n, mu, m2 = F(0), np.zeros(Cn, F), np.zeros(Cn, F)
    for r in range(world):
        nb = rec[r, 0]
        if not nb > 0:
            continue
        d, nn = rec[r, 1:1 + Cn] - mu, n + nb
        mu = mu + d * (nb / nn)
        m2 = m2 + (rec[r, 1 + Cn:] + d * d * (n * nb / nn))
        n = nn
    var = m2 / n
    invstd = F(1) / np.sqrt(var + F(1e-6))
    out = [mu, invstd, np.asarray([n], F), var]
    if mov_mean is not None:
        vm = var * (n / (n - F(1))) if unbiased and n > 1 else var
        k = F(1) - F(0.99)
        out += [mov_mean - (mov_mean - mu) * k, mov_var - (mov_var - vm) * k]
    assert all(a.dtype == F for a in out)
    return out                                        # mean, invstd, count, biased variance (, moving mean, moving variance)


def bn_merge_f64(rec):
    rec = rec.astype(np.float64)
    Cn = (rec.shape[1] - 1) // 2
    n, mu, m2 = 0.0, np.zeros(Cn), np.zeros(Cn)
    for r in range(rec.shape[0]):
        nb = rec[r, 0]
        d, nn = rec[r, 1:1 + Cn] - mu, n + nb
        mu, m2, n = mu + d * (nb / nn), m2 + rec[r, 1 + Cn:] + d * d * (n * nb / nn), nn
    return mu, m2 / n


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("Cn", [1, 8, 63, 64, 65, 1024])
def test_bn_stats_merge_piece(backend, world, Cn):
    _lib, L = _lib_bound()
    rec = _records(world, Cn, 5)
    if world >= 2:
        assert 1 in COUNTS[world] and 3932160 in COUNTS[world] and len(set(COUNTS[world])) == world
    if Cn >= 2:                                       # the case E[x^2] - E[x]^2 would lose: |mean| ~ 1e3, spread between the ranks ~ 1e-2
        assert np.abs(rec[:, 1]).min() > 900 and (world == 1 or 1e-4 < np.ptp(rec[:, 1]) < 0.2)
    rng = np.random.default_rng(9)
    mm0, mv0 = rng.normal(0, 30, Cn).astype(F), rng.uniform(0.1, 2, Cn).astype(F)
    d_rec = _dev(rec)
    worst_ulp = 0
    for unbiased in (0, 1):
        for moving in (False, True):
            d_mean, d_inv, d_cnt = (_dev(np.full(k, -7, F)) for k in (Cn, Cn, 1))
            d_mm, d_mv = (_dev(mm0), _dev(mv0)) if moving else (None, None)
            _lib.check(L.ssdr_bn_stats_merge_dev(d_rec.ptr, world, Cn, d_mean.ptr, d_inv.ptr, d_cnt.ptr, d_mm.ptr if moving else None,
                                                 d_mv.ptr if moving else None, unbiased, None))
            _lib.sync()
            want = bn_merge_np(rec, mm0 if moving else None, mv0 if moving else None, unbiased)
            got_mean, got_inv, got_cnt = d_mean.to_host(), d_inv.to_host(), d_cnt.to_host()
            assert np.array_equal(got_mean, want[0]) and np.array_equal(got_cnt, want[2]) and got_cnt[0] == sum(COUNTS[world])
            worst_ulp = max(worst_ulp, _ulps(got_inv, want[1]))
            assert np.array_equal(got_inv, want[1])                   # both builds divide and take square roots correctly rounded
            if moving:
                assert np.array_equal(d_mm.to_host(), want[4]) and np.array_equal(d_mv.to_host(), want[5])
                assert not np.array_equal(want[4], mm0) and not np.array_equal(want[5], mv0)
    ref_mu, ref_var = bn_merge_f64(rec)
    e_mu = float((np.abs(got_mean - ref_mu) / np.maximum(1.0, np.abs(ref_mu))).max())
    # the biased variance is no output of its own: it is the restatement's, which the bit-equal moving variance (unbiased = 0) pins to the kernel's
    var32 = bn_merge_np(rec, None, None, 0)[3]
    e_var = float((np.abs(var32.astype(np.float64) - ref_var) / np.maximum(1.0, np.abs(ref_var))).max())
    print("bn merge world %d C %d (%s): invstd %d ulp, mean %.2e, var %.2e of scale" % (world, Cn, backend, worst_ulp, e_mu, e_var))
    assert e_mu <= 4e-7 and e_var <= 4e-7


@pytest.mark.parametrize("world,n", [(1, 3), (2, 65), (3, 2048), (8, 129)])
def test_rank_sums_merge_piece(backend, world, n):
    _lib, L = _lib_bound()
    rng = np.random.default_rng([3, world, n])
    rec = (rng.normal(0, 1, (world, n)) * 10.0 ** rng.integers(-4, 4, (world, n))).astype(F)
    rec[:, 1] = -0.0                                   # a row of -0: 0 + (-0) is +0, in both
    want = np.zeros(n, F)
    for r in range(world):
        want = want + rec[r]
    assert want.dtype == F and not np.signbit(want[1]) and np.signbit(rec[:, 1]).all()
    d_rec, d_out = _dev(rec), _dev(np.full(n, 5, F))
    _lib.check(L.ssdr_rank_sums_merge_dev(d_rec.ptr, world, n, d_out.ptr, None))
    _lib.sync()
    assert_bits_equal(d_out.to_host(), want, "rank sums")


def test_dropout_mask_range_is_the_slice(backend):
    _lib, L = _lib_bound()
    from ssdr_al._lib import DevArray
    n, seed, step = 2 * 512 * 32, 1234567890123, 7

    def rng_(first, count):
        d = DevArray((count,), np.uint8)
        _lib.check(L.ssdr_randla_train_dropout_mask_range_dev(seed, step, first, count, d.ptr, None))
        _lib.sync()
        return d.to_host()
    whole = rng_(0, n)
    old = DevArray((n,), np.uint8)
    _lib.check(L.ssdr_randla_train_dropout_mask_dev(seed, step, n, old.ptr, None))
    _lib.sync()
    assert np.array_equal(whole, old.to_host()) and 0.45 < whole.mean() < 0.55
    for first in (0, 1, n // 2, n - 1):
        assert np.array_equal(rng_(first, n - first), whole[first:]), first
    assert not np.array_equal(rng_(2 ** 32 + 5, 4096), rng_(5, 4096))
    assert np.array_equal(rng_(2 ** 32 + 5, 4096)[1:], rng_(2 ** 32 + 6, 4095))


def test_pieces_refuse_bad_arguments(backend):
    _lib, L = _lib_bound()
    rec, a, b, c = _dev(np.ones((2, 5), F)), _dev(np.zeros(2, F)), _dev(np.zeros(2, F)), _dev(np.zeros(1, F))
    ok = [rec.ptr, 2, 2, a.ptr, b.ptr, c.ptr, None, None, 0, None]
    for hole, val in ((0, None), (3, None), (4, None), (5, None), (1, 0), (1, -1), (2, 0), (2, -3), (6, a.ptr)):
        bad = list(ok); bad[hole] = val
        assert L.ssdr_bn_stats_merge_dev(*bad) == SSDR_ERR_INVALID and L.ssdr_last_error(), (hole, val)
    out5 = _dev(np.zeros(5, F))
    oks = [rec.ptr, 2, 5, out5.ptr, None]
    for hole, val in ((0, None), (3, None), (1, 0), (2, 0)):
        bad = list(oks); bad[hole] = val
        assert L.ssdr_rank_sums_merge_dev(*bad) == SSDR_ERR_INVALID, (hole, val)
    assert L.ssdr_randla_train_dropout_mask_range_dev(1, 1, 0, 16, None, None) == SSDR_ERR_INVALID
    assert L.ssdr_randla_train_dropout_mask_range_dev(1, 1, 0, 0, a.ptr, None) == SSDR_ERR_INVALID
    _lib.sync()
    assert not a.to_host().any() and not c.to_host().any()               # nothing was launched
    assert L.ssdr_bn_stats_merge_dev(*ok) == 0
    _lib.sync()
    assert c.to_host()[0] == 2.0


# ---- children ---------------------------------------------------------------------------------------------------------------------------------------
def _gloo(tmp_path, world, port, timeout=600, **env):
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), OMP_NUM_THREADS="2", SSDR_TEST_BACKEND="gloo", **env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER]
    subprocess.run(cmd, check=True, env=env, timeout=timeout, cwd=ROOT)
    return [dict(np.load(tmp_path / ("rank%d.npz" % i))) for i in range(world)]


def _rccl_world_one(tmp_path, port, **env):
    env = dict(os.environ, SSDR_TEST_OUT=str(tmp_path), SSDR_TEST_BACKEND="nccl", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", **env)
    subprocess.run([sys.executable, WORKER], check=True, env=env, timeout=300, cwd=ROOT)
    return [dict(np.load(tmp_path / "rank0.npz"))]


# ---- 2. world 1 through the exchange is the plain trainer ----------------------------------------------------------------------------------------------
def _check_world_one(r):
    keys = sorted(k[len("plain_"):] for k in r if k.startswith("plain_") and k != "plain_exchanges")
    assert sum(k.startswith("grad|") for k in keys) > 50 and sum(k.startswith("state|") for k in keys) > 150 and sum(k.startswith("mov|") for k in keys) > 20
    for k in keys:
        assert_bits_equal(r["comm_" + k], r["plain_" + k], k)
    assert int(r["plain_steps"][0]) == 3 and int(r["plain_status"][0]) == 0 and np.isfinite(r["plain_step_losses"]).all()
    assert any(r["plain_" + k].any() for k in keys if k.startswith("grad|"))
    assert int(r["plain_exchanges"][0]) == 0
    # per call: one gather per batch-normed unit forward; backward the same, the loss's gather and the gradient sum
    n_bn = sum(k.startswith("mov|") and k.endswith("|mean") for k in keys)
    assert int(r["comm_exchanges"][0]) == 4 * (2 * n_bn + 2)
    assert int(r["mask_equal"][0]) == 1 and r["unset_exchanges"].tolist() == [0, 1]


def test_world_one_through_gloo_is_the_plain_trainer(tmp_path, emu_lib):
    _check_world_one(_gloo(tmp_path, 1, 29611, SSDR_TEST_PART="world1")[0])


@pytest.mark.gpu
def test_world_one_through_rccl_is_the_plain_trainer(tmp_path):
    from conftest import _have_gpu
    if not _have_gpu():
        pytest.skip("no GPU")
    _check_world_one(_rccl_world_one(tmp_path, 29613, SSDR_TEST_PART="world1")[0])


# ---- 3. worlds 2 and 3 against the float64 oracle over the union -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _union_oracle(flavour):
    import torch
    import _train_oracle as O
    cfg, W, batch, mask, cw, ign = WK.union_case(flavour)
    r64 = O.run(W, batch, mask, cw, ign, torch.float64)
    r32 = O.run(W, batch, mask, cw, ign, torch.float32)
    return r64, r32


def _logits_bar(r64, r32):
    return max(8 * np.abs(r32["logits"] - r64["logits"]).max(), 64 * U * np.abs(r64["logits"]).max())


def _check_gradients(x, key, flavour, what):
    """the metric and bar of test_randla_train.py::test_gradients, with the UNION's reduction rows"""
    cfg, W, batch, mask, cw, ign = WK.union_case(flavour)
    r64, r32 = _union_oracle(flavour)
    bad, worst_ratio = [], 0.0
    for (name, k), g64 in r64["grads"].items():
        g, g32 = x["%sgrad|%s|%s" % (key, name, k)], r32["grads"][(name, k)]
        assert g.shape == g64.shape and np.isfinite(g).all(), (name, k)
        scale = np.abs(g64).max()
        if k == "b" and (name, "gamma") in r64["grads"]:
            scale = np.abs(r64["grads"][(name, "W")]).max()
        m_dev, m_32 = np.abs(g - g64).max() / scale, np.abs(g32 - g64).max() / scale
        bar = max(8 * m_32, 8 * U * np.sqrt(2.0 * TC.reduction_rows(cfg, WK.UNION_B, name)))
        worst_ratio = max(worst_ratio, m_dev / bar)
        if not m_dev <= bar:
            bad.append("%-36s %-5s device %.2e float32-torch %.2e bar %.2e" % (name, k, m_dev, m_32, bar))
    print("%s: %d tensors, largest metric / bar %.2f" % (what, len(r64["grads"]), worst_ratio))
    assert not bad, "\n".join(bad)


def _check_union(r, flavour, what):
    import _train_oracle as O
    cfg, W, batch, mask, cw, ign = WK.union_case(flavour)
    r64, r32 = _union_oracle(flavour)
    signs, ties, min_var = TC.conditions(r64, r32)
    assert signs and ties, "the float32 and float64 oracle runs disagree on a sign or an arg-max set: pick another seed"
    assert min_var >= MIN_VAR
    if flavour == "sem3d":
        lab = batch["labels"]
        valid = [int((lab[lo:hi] != 0).sum()) for lo, hi in (x["tiles"] for x in r)]
        assert len(set(valid)) == len(r), "the ranks' valid counts must differ"
        assert sum(valid) == r64["valid"]
    assert [x["tiles"].tolist() for x in r][0][0] == 0 and r[-1]["tiles"][1] == WK.UNION_B
    keys = sorted(k[2:] for k in r[0] if k.startswith("a_"))
    for x in r:
        # (a) loss and accuracy: global, identical on all ranks, the oracle's to the existing loss bar
        assert_bits_equal(x["a_loss"], r[0]["a_loss"], "loss")
        assert_bits_equal(x["a_acc"], r[0]["a_acc"], "accuracy")
        assert abs(float(x["a_loss"][0]) - r64["loss"]) <= 2 * float(np.max(cw)) * _logits_bar(r64, r32)
        assert int(x["a_status"][0]) == 0 and int(x["a_step_status"][0]) == 0 and int(x["a_steps"][0]) == 3
        # (b) every gradient tensor on every rank
        _check_gradients(x, "a_", flavour, "%s rank tiles %s" % (what, x["tiles"].tolist()))
        # (c) gradients, weights, moments and moving statistics: the same bits on every rank;  (e) and again in a second run
        for k in keys:
            if k in ("tiles", "exchanges"):
                continue
            assert_bits_equal(x["a_" + k], r[0]["a_" + k], "between ranks: " + k)
            assert_bits_equal(x["b_" + k], x["a_" + k], "second run: " + k)
    moved = [k for k in keys if k.startswith("state|") and k.endswith("|W") and not np.array_equal(r[0]["a_" + k], np.asarray(W[k.split("|")[1]]["W"], F))]
    assert len(moved) > 10, "the steps must have moved the weights"
    # (d) the moving statistics after the first step (its mask is the first step mask: the statistics up to fc2 do not depend on it)
    mv = O.moving_update(W, r64["stats"])
    worst = 0.0
    for name, (mu, var) in mv.items():
        if name == "fc":
            continue
        for got, ref, old in ((r[0]["a_mov|%s|mean" % name], mu, W[name]["bn"][2]), (r[0]["a_mov|%s|var" % name], var, W[name]["bn"][3])):
            s = np.maximum(1.0, np.maximum(np.abs(ref), np.abs(old)))
            worst = max(worst, float((np.abs(got - ref) / s).max()))
    print("%s: moving statistics, worst error / scale %.3g" % (what, worst))
    assert worst <= 4e-7
    # the unbiased rule with the UNION's count: a rank's own count would sit further away than the bar on the layers of few rows
    n_l = batch["xyz"][-1].shape[1] // cfg.sub_sampling_ratio[-1]
    name = "decoder_0"
    mu_, var_, n = r64["stats"][name]
    assert n == WK.UNION_B * n_l
    assert float((0.01 * var_.numpy() * (1.0 / (n / WK.UNION_B - 1) - 1.0 / (n - 1))).max()) > 10 * 4e-7


@pytest.mark.parametrize("flavour,split,port", [("s3dis", "2,1", 29615), ("s3dis", "1,1,1", 29617), ("sem3d", "2,1", 29619), ("sem3d", "1,1,1", 29621),
                                                ("b3n360", "2,1", 29631)])        # ragged row chunks in xchg_pack_stats, on ranks with different M
def test_data_parallel_step_equals_the_union_step(tmp_path, emu_lib, flavour, split, port):
    world = len(split.split(","))
    r = _gloo(tmp_path, world, port, SSDR_TEST_PART="union", SSDR_TEST_FLAVOUR=flavour, SSDR_TEST_SPLIT=split)
    _check_union(r, flavour, "%s world %d" % (flavour, world))


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_rank_without_a_valid_row(tmp_path, emu_lib):
    """the last tile's labels are all ignored: its rank contributes zeros to the loss, no status bit, and the gradients are the union's"""
    flavour = "novalid"
    cfg, W, batch, mask, cw, ign = WK.union_case(flavour)
    assert (batch["labels"][-1] == 0).all() and (batch["labels"][:-1] != 0).any()
    r = _gloo(tmp_path, 2, 29623, SSDR_TEST_PART="union", SSDR_TEST_FLAVOUR=flavour, SSDR_TEST_SPLIT="2,1")
    r64, r32 = _union_oracle(flavour)
    for x in r:
        assert int(x["a_status"][0]) == 0 and int(x["a_step_status"][0]) == 0
        assert_bits_equal(x["a_loss"], r[0]["a_loss"], "loss")
        assert abs(float(x["a_loss"][0]) - r64["loss"]) <= 2 * float(np.max(cw)) * _logits_bar(r64, r32)
        _check_gradients(x, "a_", flavour, "no valid row on rank 1, tiles %s" % x["tiles"].tolist())


def test_no_valid_row_on_any_rank(tmp_path, emu_lib):
    r = _gloo(tmp_path, 2, 29625, SSDR_TEST_PART="union", SSDR_TEST_FLAVOUR="allinvalid", SSDR_TEST_SPLIT="2,1")
    for x in r:
        assert int(x["a_status"][0]) & 1 and int(x["a_step_status"][0]) & 1
        assert float(x["a_loss"][0]) == 0.0 and float(x["a_acc"][0]) == 0.0
        grads = [k for k in x if k.startswith("a_grad|")]
        assert len(grads) > 50 and not any(x[k].any() for k in grads)


def test_unequal_batch_counts_raise_on_every_rank(tmp_path, emu_lib):
    r = _gloo(tmp_path, 2, 29627, timeout=120, SSDR_TEST_PART="unequal")
    assert [int(x["raised"][0]) for x in r] == [1, 1]


def test_train_round_at_world_two(tmp_path, emu_lib):
    """Trainer(comm=).train_round over each rank's own TrainFeeder, two epochs: the ranks step together and end with the same bits"""
    r = _gloo(tmp_path, 2, 29629, SSDR_TEST_PART="round")
    a, b = r
    steps, want, exchanges = a["steps"].tolist()
    assert steps == want > 0 and b["steps"].tolist()[:2] == [steps, want] and exchanges > steps
    assert int(a["status"][0]) == 0 and int(b["status"][0]) == 0 and np.isfinite(a["loss"]).all()
    keys = [k for k in a if k.startswith("state|")]
    assert len(keys) > 150
    for k in keys + ["loss", "lr"]:
        assert_bits_equal(a[k], b[k], k)
    assert not np.array_equal(a["state|fc|W"], a["fc_W_start"])


class _LocalComm:
    """world 1 without a process group: what Trainer's callback needs of a Comm.  A gather of one rank is a copy (through the host: a test)."""
    rank, world, cuda = 0, 1, False

    def __init__(self, fail_at=None):
        self.calls, self.fail_at = 0, fail_at

    def raw_view(self, ptr, count, dtype=np.float32):
        from ssdr_al.distributed import RawView
        return RawView(ptr, count, dtype)

    def _count(self):
        self.calls += 1
        if self.fail_at is not None and self.calls >= self.fail_at:
            raise KeyError("the communicator fell over at call %d" % self.calls)

    def allgather_(self, a_in, a_out, stream=None):
        from ssdr_al import _lib
        self._count()
        host = np.empty(a_in.shape, np.float32)
        _lib.sync(stream)
        _lib.check(_lib.lib().ssdr_memcpy_d2h(_lib.ptr(host), a_in.ptr, host.nbytes))
        _lib.check(_lib.lib().ssdr_memcpy_h2d(a_out.ptr, _lib.ptr(host), host.nbytes))

    def allreduce_sum_(self, arr, stream=None):
        self._count()


def _small_case():
    cfg, seed = TC.Cfg3, TC.SEEDS["s3dis"]
    batch = TC.make_batch(cfg, seed)
    return cfg, TC.weights_for(cfg, seed), batch, _dev(TC.make_mask(batch, seed).reshape(-1))


def test_a_raising_callback_fails_the_call_and_the_trainer_recovers(backend):
    from ssdr_al.trainer import Trainer
    cfg, W, batch, dm = _small_case()
    dev = TC.to_device(batch)
    plain = Trainer(cfg, class_weights=TC.CLASS_W13, deterministic=True).load(W).grads_arrays(dev, mask=dm)
    want_loss, want = plain.loss(), plain.grads()
    for fail_at in (1, 40):                                               # in the first forward gather; in the middle of the backward pass
        comm = _LocalComm(fail_at)
        tr = Trainer(cfg, class_weights=TC.CLASS_W13, deterministic=True, comm=comm).load(W)
        assert tr.comm is comm
        with pytest.raises(KeyError, match="fell over at call %d" % fail_at):
            tr.grads_arrays(dev, mask=dm)
        assert comm.calls == fail_at
        assert b"exchange failed" in tr._lib.ssdr_last_error()
        tr.set_comm(None)
        assert tr.comm is None
        tr.grads_arrays(dev, mask=dm)
        assert tr.loss() == want_loss and comm.calls == fail_at
        got = tr.grads()
        for k in want:
            assert_bits_equal(got[k], want[k], str(k))
    # and a communicator that works: world 1 in this process is the plain trainer too
    comm = _LocalComm()
    tr = Trainer(cfg, class_weights=TC.CLASS_W13, deterministic=True, comm=comm).load(W).grads_arrays(dev, mask=dm)
    assert tr.loss() == want_loss and comm.calls == tr.exchanges > 0
    got = tr.grads()
    for k in want:
        assert_bits_equal(got[k], want[k], str(k))
    ws = tr.workspace_bytes()
    tr.set_comm(None)
    cmax = max(s[2] for s in tr.specs if s[4])
    assert ws - tr.workspace_bytes() == 4 * (1 + 1) * (1 + 2 * cmax)       # send [1 + 2 Cmax] and receive [world][1 + 2 Cmax]


def test_inference_forward_makes_no_exchange(backend):
    from ssdr_al import _lib
    from ssdr_al.trainer import Trainer
    cfg, W, batch, dm = _small_case()
    dev = TC.to_device(batch)
    comm = _LocalComm()
    tr = Trainer(cfg, comm=comm).load(W)
    logits, _ = tr.forward_arrays(dev, is_training=False)
    _lib.sync()
    assert comm.calls == 0 and tr.exchanges == 0
    want, _ = Trainer(cfg).load(W).forward_arrays(dev, is_training=False)
    _lib.sync()
    assert_bits_equal(logits.to_host(), want.to_host(), "inference-mode logits")
    tr.forward_arrays(dev, is_training=True, mask=dm)
    _lib.sync()
    n_bn = sum(1 for s in tr.specs if s[4])
    assert comm.calls == n_bn                                             # training mode: one gather per batch-normed unit, nothing else


def test_set_exchange_refusals(backend):
    from ssdr_al import trainer
    from ssdr_al.trainer import Trainer
    tr = Trainer(TC.Cfg3)
    L, h = tr._lib, tr._h
    cb = trainer.EXCHANGE_FN(lambda *a: 0)
    null = trainer.EXCHANGE_FN()
    rank, world = C.c_int(-1), C.c_int(-1)
    assert L.ssdr_randla_train_exchange(h, C.byref(rank), C.byref(world)) == 0 and (rank.value, world.value) == (0, 0)
    for args in ((cb, None, 0, 0), (cb, None, 0, -2), (cb, None, -1, 2), (cb, None, 2, 2), (cb, None, 5, 3), (null, None, 0, 2), (null, None, 1, 2)):
        assert L.ssdr_randla_train_set_exchange(h, *args) == SSDR_ERR_INVALID and L.ssdr_last_error(), args[2:]
    assert L.ssdr_randla_train_set_exchange(None, cb, None, 0, 1) == SSDR_ERR_INVALID
    assert L.ssdr_randla_train_exchange(h, C.byref(rank), C.byref(world)) == 0 and world.value == 0        # a refused call changes nothing
    assert L.ssdr_randla_train_set_exchange(h, cb, None, 2, 3) == 0
    assert L.ssdr_randla_train_exchange(h, C.byref(rank), C.byref(world)) == 0 and (rank.value, world.value) == (2, 3)
    assert L.ssdr_randla_train_set_exchange(h, null, None, 0, 1) == 0
    assert L.ssdr_randla_train_exchange(h, C.byref(rank), C.byref(world)) == 0 and world.value == 0


# ---- 5. / 6. ----------------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_both_libraries(emu_lib):
    from conftest import GPU_LIB
    for path in (emu_lib, GPU_LIB):
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)


def test_exchange_pieces_under_asan_ubsan():
    """a stand-alone program (tests/san/train_exchange_main.cpp) linked with the sanitized objects of the CPU logic build: the packs, both merges and
    the range-table zeroing at world 3 over exactly sized arrays, against scalar loops; no report"""
    from conftest import PKG
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(PKG, "csrc"), "train-exchange-san"])
    env = dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "san", "train_exchange_san")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert "train exchange ok" in r.stdout
