"""Worker of tests/test_train_exchange.py, and the cases the two share: one rank of a data-parallel training run (Trainer(comm=)).
SSDR_TEST_BACKEND=gloo: the CPU logic build; nccl: world 1 on the GPU through RCCL.  SSDR_TEST_PART:
  "world1"   Trainer(deterministic=True, comm=comm) against Trainer(deterministic=True) in the same process, on the s3dis case of _train_cases;
  "union"    this rank's tiles of a B = 3 union batch (SSDR_TEST_FLAVOUR, SSDR_TEST_SPLIT = tiles per rank, e.g. "2,1"), run twice;
  "unequal"  train_round with feeders whose batch counts differ between the ranks;
  "round"    train_round over a TrainFeeder of this rank's own clouds, two epochs.
Every rank writes rank<r>.npz."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ssdr-al_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _train_cases as TC  # noqa: E402

# seeds for which _train_cases.conditions() holds for the union batch (float64 and float32 agree on every activation sign and pooling tie set; no
# degenerate batch norm), found on the CPU; test_train_exchange.py asserts the conditions again
UNION_SEEDS = {"s3dis": 3, "sem3d": 7}
UNION_B = 3
STEP_MASK_SEEDS = (100, 101, 102)


@functools.lru_cache(maxsize=None)
def union_case(flavour):
    """(cfg, weights, union batch [B = 3], dropout mask of the gradient call, class weights, ignored labels) of a flavour:
    s3dis (class weights), sem3d (label 0 ignored: the ranks' valid counts differ), novalid (sem3d with the LAST tile's labels all ignored),
    allinvalid (sem3d with every label ignored)"""
    if flavour in TC.PATH_CASES:              # a case of tests/test_train_paths.py at B = 3: ranks with different row counts, none a power of two
        cfg, kw, cw, ign = TC.PATH_CASES[flavour]
        assert cfg.batch_size == UNION_B and cfg.num_classes == 13
        seed = TC.SEEDS[flavour]
        batch = TC.make_batch(cfg, seed, **kw)
        return cfg, TC.weights_for(cfg, seed), batch, TC.make_mask(batch, seed), TC.CLASS_W13, ign
    base = "s3dis" if flavour == "s3dis" else "sem3d"
    seed = UNION_SEEDS[base]
    if base == "s3dis":
        cfg, kw, cw, ign = TC.Cfg3, {}, TC.CLASS_W13, ()
    else:
        cfg, kw, cw, ign = TC.Cfg3Sem, dict(n_labels=9), np.linspace(0.6, 1.8, 8).astype(np.float32), (0,)
    W = TC.weights_for(cfg, seed)
    batch = TC.make_batch(cfg, seed, B=UNION_B, **kw)
    if flavour == "novalid":
        batch["labels"][-1] = 0
    elif flavour == "allinvalid":
        batch["labels"][:] = 0
    return cfg, W, batch, TC.make_mask(batch, seed), cw, ign


def tiles(batch, lo, hi):
    """tiles lo .. hi - 1 of a host batch (the pyramid's indices are per tile)"""
    return {k: ([np.ascontiguousarray(a[lo:hi]) for a in v] if isinstance(v, list) else np.ascontiguousarray(v[lo:hi])) for k, v in batch.items()}


def mask_rows(mask, batch, lo, hi):
    n = batch["labels"].shape[1]
    return np.ascontiguousarray(mask[lo * n:hi * n])


def full_state(tr):
    """weights, the moving statistics and Adam's moments, flat: {"scope|key": array}"""
    st, out = tr.state(), {}
    for name, ent in st["weights"].items():
        out[name + "|W"] = ent["W"]
        if ent["b"] is not None:
            out[name + "|b"] = ent["b"]
        if ent["bn"] is not None:
            for k, a in zip(("gamma", "beta", "mean", "var"), ent["bn"]):
                out[name + "|" + k] = a
    for (name, key), (m, v) in st["adam"].items():
        out["%s|%s|m" % (name, key)], out["%s|%s|v" % (name, key)] = m, v
    return out


def _dev_mask(mask):
    from ssdr_al._lib import DevArray
    return DevArray.from_host(np.ascontiguousarray(mask, np.uint8).reshape(-1))


def run_trainer(res, key, cfg, W, batch, masks, cw, ign, comm):
    """grads_arrays with masks[0], then one step per mask of masks[1:]; what the test compares lands in res under key"""
    from ssdr_al.trainer import Trainer
    tr = Trainer(cfg, class_weights=cw, ignored_labels=ign, deterministic=True, comm=comm).load(W)
    assert tr.comm is comm
    dev = TC.to_device(batch)
    tr.grads_arrays(dev, mask=_dev_mask(masks[0]))
    res[key + "loss"], res[key + "acc"] = np.asarray([tr.loss()], np.float32), np.asarray([tr.accuracy()], np.float32)
    res[key + "status"] = np.asarray([tr.status()])
    for (name, k), g in tr.grads().items():
        res["%sgrad|%s|%s" % (key, name, k)] = g
    losses = []
    for t, m in enumerate(masks[1:]):
        tr.step_arrays(dev, mask=_dev_mask(m))
        losses.append(tr.loss())
        if t == 0:
            for name, ent in tr.weights().items():
                if ent["bn"] is not None:
                    res["%smov|%s|mean" % (key, name)], res["%smov|%s|var" % (key, name)] = ent["bn"][2], ent["bn"][3]
    res[key + "step_losses"] = np.asarray(losses, np.float32)
    res[key + "step_status"] = np.asarray([tr.status()])
    res[key + "steps"] = np.asarray([tr.step_count()])
    res[key + "exchanges"] = np.asarray([tr.exchanges])
    for k, a in full_state(tr).items():
        res["%sstate|%s" % (key, k)] = a
    return tr


def part_world1(comm, rank, world, res):
    cfg, seed = TC.Cfg3, TC.SEEDS["s3dis"]
    W, batch = TC.weights_for(cfg, seed), TC.make_batch(cfg, seed)
    masks = [TC.make_mask(batch, seed)] + [TC.make_mask(batch, s) for s in STEP_MASK_SEEDS]
    run_trainer(res, "plain_", cfg, W, batch, masks, TC.CLASS_W13, (), None)
    tr = run_trainer(res, "comm_", cfg, W, batch, masks, TC.CLASS_W13, (), comm)
    # the generated mask of rank 0 of an equal-share run is the plain trainer's, and set_comm(None) takes the hook out again
    from ssdr_al.trainer import Trainer
    a = tr.make_mask(2, 512, step=5).to_host()
    b = Trainer(cfg, seed=tr.seed).make_mask(2, 512, step=5).to_host()
    res["mask_equal"] = np.asarray([int(np.array_equal(a, b))])
    before = tr.exchanges
    tr.set_comm(None)
    tr.grads_arrays(TC.to_device(batch), mask=_dev_mask(masks[0]))
    res["unset_exchanges"] = np.asarray([tr.exchanges - before, int(tr.comm is None)])


def part_union(comm, rank, world, res):
    flavour = os.environ["SSDR_TEST_FLAVOUR"]
    split = [int(x) for x in os.environ["SSDR_TEST_SPLIT"].split(",")]
    assert len(split) == world and sum(split) == UNION_B
    lo, hi = sum(split[:rank]), sum(split[:rank + 1])
    cfg, W, batch, mask, cw, ign = union_case(flavour)
    masks = [mask] + [TC.make_mask(batch, s) for s in STEP_MASK_SEEDS]
    mine, my_masks = tiles(batch, lo, hi), [mask_rows(m, batch, lo, hi) for m in masks]
    res["tiles"] = np.asarray([lo, hi])
    for run in ("a_", "b_"):
        run_trainer(res, run, cfg, W, mine, my_masks, cw, ign, comm)


def part_unequal(comm, rank, world, res):
    from ssdr_al.trainer import Trainer

    class Feeder:                                   # a feeder is asked for its batch count before it is asked for a batch
        steps_per_epoch = 2 + rank

        def epoch_batches(self, stream=None):
            raise AssertionError("train_round went on to step although the batch counts differ")
    tr = Trainer(TC.Cfg3, comm=comm).load(TC.weights_for(TC.Cfg3, 1))
    try:
        tr.train_round(Feeder(), 2)
        res["raised"] = np.asarray([0])
    except ValueError as e:
        res["raised"] = np.asarray([int("batches per epoch" in str(e))])


def part_round(comm, rank, world, res):
    from ssdr_al import training
    from ssdr_al.helper_tool import ConfigS3DIS
    from ssdr_al.trainer import Trainer

    class Small(ConfigS3DIS):
        num_points = 512
        num_layers = 3
        sub_sampling_ratio = [4, 4, 2]
        d_out = [16, 64, 128]
        batch_size = 2
        train_steps = 2
        num_classes = 13
    rng = np.random.default_rng(50 + rank)           # every rank its own clouds, the same number of them
    clouds, pg = [], []
    for n in (300, 800, 1300):
        lab = rng.integers(0, 13, n).astype(np.int32)
        clouds.append(dict(xyz=(rng.random((n, 3)) * [4, 4, 2]).astype(np.float32), rgb=rng.random((n, 3)).astype(np.float32), labels=lab))
        pg.append(np.stack([(rng.random(n) < 0.5).astype(np.float32), lab.astype(np.float32)]))
    feeder = training.TrainFeeder(clouds, pg, config=Small, dataset="S3DIS", seed=50 + rank)
    W = TC.weights_for(Small, 6)
    tr = Trainer(Small, seed=3, deterministic=True, comm=comm).load(W)
    res["result"] = np.asarray(tr.train_round(feeder, 2), np.float64)
    res["loss"], res["status"] = np.asarray([tr.loss()], np.float32), np.asarray([tr.status()])
    res["steps"] = np.asarray([tr.step_count(), 2 * feeder.steps_per_epoch, tr.exchanges])
    res["lr"] = np.asarray([tr.lr])
    res["fc_W_start"] = np.asarray(W["fc"]["W"], np.float32)
    for k, a in full_state(tr).items():
        res["state|" + k] = a
    feeder.close()


def main():
    import torch.distributed as dist
    backend = os.environ.get("SSDR_TEST_BACKEND", "gloo")
    if backend == "nccl":
        import torch
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from ssdr_al import _lib
    from ssdr_al.distributed import Comm
    if backend == "gloo":
        _lib.use(os.path.join(ROOT, "tests", "hipemu", "libssdr_al_emu.so"))
    else:
        _lib.check(_lib.lib().ssdr_init(0))
    comm = Comm(dist, "cuda" if backend == "nccl" else "cpu")
    res = {}
    {"world1": part_world1, "union": part_union, "unequal": part_unequal, "round": part_round}[os.environ["SSDR_TEST_PART"]](comm, rank, world, res)
    np.savez(os.path.join(os.environ["SSDR_TEST_OUT"], "rank%d.npz" % rank), **res)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
