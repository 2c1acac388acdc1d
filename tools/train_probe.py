"""One RandLA-Net training step (ssdr_al.trainer.Trainer) at the workload's shape, B = 6 tiles of N = 40 960 points, on batches a TrainFeeder cuts
from synthetic S3DIS-like rooms (synthetic.make_room, sub-sampled at 0.04 m).  GPU only; not part of bench.py.

Without arguments the tool is a driver: it starts itself twice as a child process, each under its own `timeout`,
  1. `--child time`: warm-up steps, then timed steps; the forward / loss + backward / update split comes from HIP events on the step's stream
     (ssdr_randla_train_last_ms), the step time from a host clock around steps that end in a stream synchronise;
  2. `--child trace` under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host), from whose kernel statistics the ten
     slowest kernels are listed;
and prints one JSON line.  With --deterministic the timed child measures the step in BOTH modes in the same process (the default atomic scatters
first, then Trainer.set_deterministic(True) on the same trainer and batch: forward / backward / update for each, and the workspace), and the traced
child runs in deterministic mode: from the per-dispatch kernel trace of its last step comes the share of the step's kernel time that the list
builds (key generation, the radix sort, the offsets) and the two reductions take.  The FLOP count is computed from the shapes (every dense layer: 2 M in out forward, the same again for dW and for dX
where the input has a gradient; the attention softmax and the other element-wise work are not counted) and set against the float32 vector and
matrix peaks of the MI355X, which are the same 157.3 TFLOP/s.
With --comm only the timed child runs: it measures the hook-less step, then joins an RCCL process group of world 1 in the same process, sets it on
the SAME trainer (Trainer.set_comm) and measures the data-parallel step: forward / backward / update, the collectives per step, and the host's
enqueue time per step (until step_arrays returns) beside the step's time on the GPU: while the first is the smaller one the callbacks run ahead of
the GPU's queue and their cost on the host is hidden.
Usage: python tools/train_probe.py [--deterministic | --comm] [--rooms 8] [--steps 5] [--warmup 2] [--points 40960] [--batch 6] [--out bench_out/train_probe]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F32 = 157.3e12          # vector and matrix (v_mfma_f32_*_f32) alike


def dense_flops(cfg, B, specs):
    """(forward, backward) FLOPs of the dense layers of one step, from the shapes"""
    N = [cfg.num_points]
    for r in cfg.sub_sampling_ratio:
        N.append(N[-1] // r)
    L, K = cfg.num_layers, cfg.k_n
    fwd = bwd = 0.0
    for name, cin, cout, bias, bn, act, tr in specs:
        if name.startswith("Encoder_layer_"):
            lvl = int(name[len("Encoder_layer_")])
            per_nb = name.endswith(("LFAmlp1", "LFAmlp2", "LFAatt_pooling_1fc", "LFAatt_pooling_2fc"))
            rows = B * N[lvl] * (K if per_nb else 1)
        elif name == "decoder_0":
            rows = B * N[L]
        elif name.startswith("Decoder_layer_"):
            rows = B * N[L - 1 - int(name[len("Decoder_layer_"):])]
        else:
            rows = B * N[0]
        f = 2.0 * rows * cin * cout
        fwd += f
        bwd += f if name == "fc0" or name.endswith("LFAmlp1") else 2 * f         # dW always, dX unless the input is data
    return fwd, bwd


def child(mode, a):
    from ssdr_al import _lib, subsampling, synthetic, training
    from ssdr_al.helper_tool import ConfigS3DIS
    from ssdr_al.trainer import Trainer
    class cfg(ConfigS3DIS):
        num_points = a.points
        batch_size = a.batch
    if a.comm and mode == "time":                    # the framework takes the device first, as in the sharded round's workers: one HIP runtime per process
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    _lib.check(_lib.lib().ssdr_init(0))
    rooms = []
    for i in range(a.rooms):
        xyz, rgb, lab = synthetic.make_room(40000 + i, density=2000.0)
        sp, sc, sl = subsampling.compute(xyz, features=rgb.astype(np.float32), classes=lab.astype(np.int32), sampleDl=0.04)
        rooms.append(dict(xyz=sp, rgb=sc, labels=sl.reshape(-1).astype(np.int32)))
    r = np.random.default_rng(1)
    pg = [np.stack([(r.random(len(c["xyz"])) < 0.3), c["labels"]]).astype(np.float32) for c in rooms]
    feeder = training.TrainFeeder(rooms, pg, config=cfg, dataset="S3DIS", color_scale=1.0 / 255.0)
    tr = Trainer(cfg).load(synthetic.init_weights(0, trained_like=False))
    batch = feeder.next_batch(None)
    assert batch.size == cfg.batch_size, "need at least batch_size rooms"
    arrays = batch.arrays                       # the same batch every step: the step's time does not depend on the values
    steps = a.steps if mode == "time" else 1
    med = lambda v: float(np.median(v))

    def timed():
        for _ in range(a.warmup):
            tr.step_arrays(arrays)
        _lib.sync()
        split, wall = [], []
        del enqueue[:]
        for _ in range(steps):
            t0 = time.perf_counter()
            tr.step_arrays(arrays)
            enqueue.append(1e3 * (time.perf_counter() - t0))
            _lib.sync()
            wall.append(1e3 * (time.perf_counter() - t0))
            split.append(tr.last_ms())
        return split, wall
    enqueue = []
    if a.deterministic and mode == "trace":
        tr.set_deterministic(True)
    split, wall = timed()
    det = None
    if a.deterministic and mode == "time":           # the same trainer, the same batch, the other mode
        ws_default = tr.workspace_bytes()
        tr.set_deterministic(True)
        dsplit, dwall = timed()
        det = dict(step_ms_events=round(med([sum(s) for s in dsplit]), 3), step_ms_host=round(med(dwall), 3),
                   forward_ms=round(med([s[0] for s in dsplit]), 3), backward_ms=round(med([s[1] for s in dsplit]), 3), update_ms=round(med([s[2] for s in dsplit]), 3),
                   workspace_gib=round(tr.workspace_bytes() / 2.0 ** 30, 3), workspace_growth_mib=round((tr.workspace_bytes() - ws_default) / 2.0 ** 20, 1))
    plain_enqueue = med(enqueue)
    dp = None
    if a.comm and mode == "time":                    # the same trainer, the same batch, through RCCL at world 1
        from ssdr_al.distributed import Comm
        tr.set_comm(Comm(dist, "cuda"))
        before = tr.exchanges
        csplit, cwall = timed()
        per_step = (tr.exchanges - before) // (a.warmup + steps)
        dp = dict(world=1, step_ms_events=round(med([sum(s) for s in csplit]), 3), step_ms_host=round(med(cwall), 3), host_enqueue_ms=round(med(enqueue), 3),
                  forward_ms=round(med([s[0] for s in csplit]), 3), backward_ms=round(med([s[1] for s in csplit]), 3), update_ms=round(med([s[2] for s in csplit]), 3),
                  collectives_per_step=int(per_step), workspace_gib=round(tr.workspace_bytes() / 2.0 ** 30, 3))
        tr.set_comm(None)
        _lib.sync()
        dist.destroy_process_group()
    loss = tr.loss()
    assert np.isfinite(loss) and tr.status() == 0
    fwd, bwd = dense_flops(cfg, cfg.batch_size, tr.specs)
    step_ms = med([sum(s) for s in split])
    out = dict(mode=mode, deterministic=bool(tr.deterministic) if det is None else None, deterministic_mode=det, B=cfg.batch_size, N=cfg.num_points, steps=steps, warmup=a.warmup, loss=loss,
               step_ms_events=round(step_ms, 3), step_ms_host=round(med(wall), 3), host_enqueue_ms=round(plain_enqueue, 3), data_parallel=dp,
               forward_ms=round(med([s[0] for s in split]), 3), backward_ms=round(med([s[1] for s in split]), 3), update_ms=round(med([s[2] for s in split]), 3),
               dense_gflop=dict(forward=round(fwd / 1e9, 2), backward=round(bwd / 1e9, 2)),
               tflops=round((fwd + bwd) / (step_ms * 1e-3) / 1e12, 3), share_of_f32_peak=round((fwd + bwd) / (step_ms * 1e-3) / PEAK_F32, 4),
               workspace_gib=round((tr.workspace_bytes() if det is None else ws_default) / 2.0 ** 30, 3))
    batch.release(None)
    feeder.close()
    print("TRAIN_PROBE " + json.dumps(out))


def slowest_kernels(out_dir, n=10):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    rows = []
    with open(sorted(files)[-1]) as f:
        for row in csv.DictReader(f):
            rows.append(dict(kernel=row.get("Name", "")[:90], calls=int(row.get("Calls", 0)), total_ms=round(float(row.get("TotalDurationNs", 0)) / 1e6, 3),
                             percent=float(row.get("Percentage", 0))))
    rows.sort(key=lambda r: -r["total_ms"])
    return rows[:n]


LIST_KERNELS = ("inv_keys_kernel", "inv_off_kernel", "::rs_")                       # the list builds: keys, the radix sort's kernels, offsets
REDUCE_KERNELS = ("rows_reduce_kernel", "pool_share_kernel", "pool_reduce_kernel")  # the two reductions


def deterministic_share(out_dir):
    """share of the LAST step's kernel time (per-dispatch kernel trace; a step ends with its adam_kernel dispatch) spent in the list builds and in
    the two reductions"""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    with open(sorted(files)[-1]) as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    ends = [i for i, r in enumerate(rows) if "adam_kernel" in r[0]]
    if len(ends) < 2:
        return None
    step = rows[ends[-2] + 1:ends[-1] + 1]
    total = sum(e - s for _, s, e in step)
    part = lambda names: sum(e - s for n, s, e in step if any(k in n for k in names))
    lists, red = part(LIST_KERNELS), part(REDUCE_KERNELS)
    return dict(step_kernel_ms=round(total / 1e6, 3), dispatches=len(step), list_build_ms=round(lists / 1e6, 3), reductions_ms=round(red / 1e6, 3),
                list_build_share=round(lists / total, 4), reductions_share=round(red / total, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=40960)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "train_probe"))
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--deterministic", action="store_true", help="time both modes; trace the deterministic one")
    ap.add_argument("--comm", action="store_true", help="time the step through RCCL at world 1 against the hook-less step, in the same process")
    ap.add_argument("--port", type=int, default=29631)
    ap.add_argument("--child", choices=["time", "trace"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a)
    os.makedirs(a.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--rooms", str(a.rooms), "--steps", str(a.steps), "--warmup", str(a.warmup), "--points", str(a.points),
          "--batch", str(a.batch)] + (["--deterministic"] if a.deterministic else []) + (["--comm"] if a.comm else [])
    result = {}
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1") if a.comm else None
    runs = (("time", []), ("trace", ["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "train", "--output-format", "csv", "--"]))
    for mode, prefix in runs[:1] if a.comm else runs:
        cmd = ["timeout", "-k", "10", str(a.limit)] + prefix + me + ["--child", mode]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        with open(os.path.join(a.out, "child_%s.log" % mode), "w") as f:
            f.write(p.stdout)
        if p.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            print(json.dumps(dict(probe="train", failed=mode, returncode=p.returncode, log=os.path.join(a.out, "child_%s.log" % mode))))
            return 1
        line = [l for l in p.stdout.splitlines() if l.startswith("TRAIN_PROBE ")]
        result[mode] = json.loads(line[-1][len("TRAIN_PROBE "):]) if line else None
    if a.comm:
        print(json.dumps(dict(probe="train", timed=result["time"])))
        return 0
    print(json.dumps(dict(probe="train", timed=result["time"], traced_step_ms=(result["trace"] or {}).get("step_ms_events"), slowest_kernels=slowest_kernels(a.out),
                          deterministic_share=deterministic_share(a.out) if a.deterministic else None)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
