"""The hot path end to end, device-resident: grid-subsample -> tile -> KNN pyramid -> RandLA-Net inference ->
uncertainty / region statistics -> candidate features -> per-cloud chamfer graph + propagation -> FPS selection.

This is the sequencing the reference spreads over data_prepare_s3dis.py:58, s3dis_dataset.py:115-183,
sampler2.py:580-642 (prediction) and :736-781 (the gcn_fps branch of sampling); files, pickles and the label
simulation are out of scope.  All arithmetic happens in libssdr_al.so; the host only moves small index lists."""
import ctypes as C
import os
import time

import numpy as np

from . import _lib, knn, randlanet, sampler, synthetic
from ._lib import DevArray
from .helper_tool import ConfigS3DIS


class _Pairs:
    """A read-only sequence of (a[i], b[i]) integer pairs that behaves like the list of tuples it stands for (indexing, slicing, iteration, len, ==) and
    builds that list only when asked to: an AL round hands back 20 000 candidates and 10 000 picks, and building 30 000 Python tuples nobody may look at
    cost the collect 1.5 of its 2.2 ms."""
    __slots__ = ("a", "b", "_list")

    def __init__(self, a, b):
        self.a, self.b, self._list = np.asarray(a), np.asarray(b), None

    def tolist(self):
        if self._list is None:
            self._list = list(zip(self.a.tolist(), self.b.tolist()))
        return self._list

    def __len__(self):
        return len(self.a)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.tolist()[i]
        return (int(self.a[i]), int(self.b[i]))

    def __iter__(self):
        return iter(self.tolist())

    def __eq__(self, other):
        return self.tolist() == (other.tolist() if isinstance(other, _Pairs) else other)

    def __repr__(self):
        return repr(self.tolist())


SELECTORS = ("fps", "kcenter", "edcd", "topk", "coregcn", "random", "all")
REGION_SAMPLERS = ("random", "all")      # no scoring, no network outputs: RandomSampler / AllSampler (sampler2.py:410-520)

# The words of the selection chains' int32 result buffers that the host reads.  include/ssdr_al.h defines them: d_result in the comment above
# ssdr_gcn_fps_sampling_dev (the edcd and topk chains share its header), d_plan in the one above ssdr_gcn_fps_sharded_local_dev.
RES_N_UNL, RES_N_PICKS, RES_STATUS = 0, 4, 5      # d_result: the candidates, the picks, the status bits
RES_HEADER = 8                                    # the picks start here; the candidate list follows at RES_HEADER + max_select
PLAN_N_ALL, PLAN_OVERFLOW = 8, 9                  # d_plan ([0..7] as d_result, [RES_N_PICKS] = all ranks' picks): all ranks' candidates; a rank offers more than nu_max
PLAN_HEADER = 16                                  # the candidates per rank start here


def _plan_gcand(world, nu_max):
    """where d_plan's global candidate list starts: behind the header, the counts per rank and the rows of the gathered array"""
    return PLAN_HEADER + world + world * nu_max


def _host_rule():
    """SSDR_SELECT_HOST_RULE: the candidate rule runs on the host (the tests' reference for the device rule)"""
    return bool(os.environ.get("SSDR_SELECT_HOST_RULE"))


def _capacities(nvalid, nlab, batch):
    """What the candidate rule can produce at most when `batch` regions are asked of clouds with `nvalid` ranked and `nlab` labelled regions each:
    (picks, cap_unl, share, cap_rows, cap_nmax, cap_sq) — the picks, the candidates, what a cloud can offer, the rows (candidates + labelled), the largest
    cloud's rows and the sum of the clouds' squared rows.  The four cap_* size buffers and are at least 1."""
    picks = int(min(batch, nvalid.sum()))
    cap_unl = int(min(2 * picks, nvalid.sum()))
    share = np.minimum(2 * picks, nvalid)                    # a cloud offers at most 2 x (its top regions) <= 2 x picks, and what it has
    # the largest sum of squared cloud shares: fill the roomiest clouds first
    left, sq = cap_unl, 0
    for i in np.argsort(-(share + nlab), kind="stable"):
        a = int(min(share[i], left)); left -= a
        sq += (a + int(nlab[i])) ** 2
    return picks, max(cap_unl, 1), share, max(cap_unl + int(nlab.sum()), 1), max(int((share + nlab).max()) if len(share) else 1, 1), max(int(sq), 1)


class _Issued:
    """One issued selection: _select_issue fills it, _select_collect consumes it and keeps the last one (comb_all, label_selected's communicator).
    route: "device" (a one-call chain's d_result in `buf`, its picks' capacity in `max_select`), "sharded" (d_plan and the replicated picks), "topk" (`buf`
    in the top's layout) or "host" (`picks`: a host array, or the device array the chain fills).  pairs: the candidates as (cloud, region); rooms / spin:
    their (room id, superpoint in room), for the sharded fps / k-center routes over the GLOBAL candidate list.  keep: temporaries the enqueued chain reads.
    Sharded extras: emu_mod (SSDR_EMULATE_WORLD: the picks index repeated rows), gcand (the global candidate list) and gorder (the global ranking) for the
    host rule's labelling, comb / comb_n (the gathered features behind comb_all)."""
    __slots__ = ("route", "comm", "buf", "max_select", "picks", "pairs", "rooms", "spin", "keep", "emu_mod", "gcand", "gorder", "comb", "comb_n")

    def __init__(self, route, comm=None, buf=None, max_select=0):
        self.route, self.comm, self.buf, self.max_select = route, comm, buf, int(max_select)
        self.picks = self.pairs = self.rooms = self.spin = self.gcand = self.gorder = self.comb = None
        self.keep, self.emu_mod, self.comb_n = [], 0, 0


class _Picks:
    """Where the picks of a collected selection lie, for label_selected.  layout HOST: `items` (region ids, made on the host); RESULT0 / RESULT1: in `buf`,
    a one-call chain's d_result / the top's (the numbers are ssdr_oracle_label_items_dev's `layout`), `max_select` its picks' capacity; REPLICATED: the
    sharded fps / k-center chain's replicated picks over the global candidate list `gcand`.  A sharded selection adds `own` (this rank's picks: their
    positions among all picks) and, for HOST, the 64-bit walk `keys`; `refuse`: why these picks cannot be labelled."""
    HOST, RESULT0, RESULT1, REPLICATED = -1, 0, 1, 2
    __slots__ = ("layout", "buf", "max_select", "items", "keys", "own", "gcand", "refuse")

    def __init__(self, layout, buf=None, max_select=0, items=None, keys=None, own=None, gcand=None, refuse=None):
        self.layout, self.buf, self.max_select, self.items, self.keys, self.own, self.gcand, self.refuse = layout, buf, int(max_select), items, keys, own, gcand, refuse


def selector_for(sampler_args, trained_gcn=False):
    """The selector that runs the branch of TSampler.sampling() a reference `sampler_args` names, tested in the reference's elif order
    (sampler2.py:670, :687, :736, :783): "edcd", "gcn", "gcn_fps", else uncertainty alone.  The "gcn" branch trains a GCN during selection (minutes in
    the reference): it is named only on request — trained_gcn=True returns "coregcn" for it, the default keeps refusing it."""
    args = list(sampler_args)
    if "edcd" in args:
        return "edcd"
    if "gcn" in args and trained_gcn:
        return "coregcn"
    if "gcn" in args:
        raise ValueError('sampler_args names the "gcn" branch (a GCN trained during selection, sampler2.py:687-734), which is out of scope here; '
                         'selector="kcenter" runs its last step (kCenterGreedy over candidates + labelled regions), and selector_for(args, trained_gcn=True) '
                         'names the selector that trains the GCN ("coregcn")')
    if "gcn_fps" in args:
        return "fps"
    return "topk"


class HotPath:
    def __init__(self, weights, config=ConfigS3DIS, sampler_args=("sb", "WetSU", "clsbal", "gcn_fps"), gcn_number=1, gcn_top=0,
                 select_per_tile=37, labeled_per_tile=15, seed=0, precision="f32", selector="fps", tiles32=True, min_size=1, round_num=5,
                 label_seed=None, batch_size=None, max_size=None, chamfer_mode="f64", gcn_steps=20000, gcn_dropout=0.3, gcn_seed=0, gcn_form="auto",
                 draws="device", draw_seed=0, max_iter=32, total_num=None, draw_key_bits=32):
        self.cfg = config
        self.net = None if weights is None else randlanet.Network(config).load(weights).set_precision(precision).set_formulation(tiles32)
        self.sampler_args = list(sampler_args)
        self.gcn_number, self.gcn_top = gcn_number, gcn_top
        self.select_per_tile, self.labeled_per_tile = select_per_tile, labeled_per_tile
        self.batch_size = None if batch_size is None else int(batch_size)      # sampling()'s batch_size outright (default: select_per_tile x clouds)
        self.seed = seed
        # min_size: regions of fewer points are neither ranked nor used as labelled rows (sampler2.py:616, :628; the reference's default is 1);
        # round_num: the class-balanced draw of the labelled rows takes (round_num - 1) * 1000 of the labelled regions (sampler2.py:297-302; SURVEY
        # section 8d quotes the workload at round 5); label_seed seeds NumPy's legacy generator for that draw (the reference draws from np.random)
        # max_size: the Semantic3D flavour also drops regions of more than 1000 points from both populations (SSRD_AL_semantic3d/sampler2.py:644, :655)
        self.max_size = None if max_size is None else int(max_size)
        # chamfer_mode: "f64" (S3DIS, fps_gcn_cpu.create_cd) or "f32_cuda" (the Semantic3D code's create_cd_cuda values, fps_gcn_cuda.py:13-30)
        self.chamfer_mode = {"f64": 0, "f32_cuda": 1}[chamfer_mode]
        self.min_size, self.round_num = int(min_size), int(round_num)
        self.label_seed = int(seed if label_seed is None else label_seed)
        # "fps": farthest_features_sample over the candidates' propagated features (the gcn_fps branch, sampler2.py:736-781);
        # "kcenter": kCenterGreedy.select_batch_ over candidates + labelled regions with the labelled ones as already selected
        # (the step the reference's gcn branch ends with, gcn.py:247, kcenterGreedy.py:60-128; BASELINE configuration 4's global k-center);
        # "edcd": every cloud's farthest_superpoint_sample over its candidates (sampler2.py:670-685, :49-80), always with the float64 chamfer;
        # "topk": the first batch_size regions of the ranking (sampler2.py:783-806).  selector_for() maps a reference sampler_args to one of them
        # "coregcn": the reference's "gcn" branch (sampler2.py:687-734 -> gcn.py:193-263): create_adj, gcn_steps Adam steps of the two-layer GCN (20 000 on
        # S3DIS, 2 000 on Semantic3D) from the weights gcn_seed draws, dropout gcn_dropout, then kCenterGreedy over the trained 129-d rows
        assert selector in SELECTORS, "selector must be one of %s" % (SELECTORS,)
        self.selector = selector
        self.gcn_steps, self.gcn_dropout, self.gcn_seed, self.gcn_form = int(gcn_steps), float(gcn_dropout), int(gcn_seed), gcn_form
        # "random" / "all": RandomSampler / AllSampler (sampler2.py:455-520, :410-453) — no scoring; SeedSampler is seed_round().  draws: "device" (counter-based,
        # a function of (draw_seed, round_num, iteration); csrc/select_random.hip) or "host" (draw_rng, a np.random.RandomState consumed as the reference
        # consumes np.random); max_iter: where the loop stops when only regions below min_size are left; total_num: the samplers' total_num (default: S)
        assert draws in ("device", "host"), 'draws must be "device" or "host"'
        self.draws, self.draw_seed, self.max_iter, self.draw_key_bits = draws, int(draw_seed), int(max_iter), int(draw_key_bits)
        self.total_num = None if total_num is None else int(total_num)
        self.draw_rng = np.random.RandomState(self.draw_seed & 0xffffffff) if draws == "host" else None
        self._unl_lists = None      # draws="host": every cloud's unlabelled list in the reference's order (local ids), kept across rounds
        self._pred_resident = False # predicted classes (self.cls) are those of a prediction pass over the resident outputs
        self.record_shares = False  # device draws: read every iteration's each_file_number back too (LabelResult.draw_info; the tests)
        self._drawn0 = None         # iteration 0 of a "random" / "all" round, drawn by step_selection()
        self.fps_start = 0          # np.random.randint(0, n) in the reference (fps_gcn_cpu.py:133); fixed here
        self.stream = None          # stream of the pyramid .. scoring stages (None = the library's main stream)
        self.front_stream = None    # stream of the front end (grid-subsample + tiles)
        self.knn_stream = None      # stream of the KNN pyramid (None = self.stream)
        self.score_stream = None    # stream of the scoring stage (None = self.stream)
        self.sel_stream = None      # stream of the selection chain (None = the library stream)
        self.pipelined = False      # set by Pipelined: later batches are in flight on the stage streams when a selection is collected
        self.global_order = None
        self._dist = None           # a sharded run's static tables (_dist_setup)
        self._pending = None        # the issued, not yet collected selection (_Issued)
        self._collected = None      # the last collected one
        self._last_sel = None       # where its picks lie (_Picks) until label_selected has spent them
        self.rooms = []
        self.timing = None
        self.pt_off = None          # where every cloud's points start in the concatenated arrays (LabelResult.to_host per cloud)
        self.pseudo_mask = self.pseudo_label = None      # the two rows of pseudo_gt over all points, resident across rounds (label_selected)
        self._room_plan = self._room_plan_lib = None      # the loaded rooms' plan (ssdr_rooms_plan_create_dev) and the library that owns it

    def _drop_room_plan(self):
        plan, L = self._room_plan, self._room_plan_lib
        self._room_plan = self._room_plan_lib = None
        if plan is not None:
            _lib.check(L.ssdr_rooms_plan_destroy(plan))

    def close(self):
        """frees what the library keeps for this object beyond its arrays: the loaded rooms' plan (waits for the device)"""
        self._drop_room_plan()

    def __del__(self):
        try:
            self._drop_room_plan()
        except Exception:
            pass

    # ---- setup (untimed): upload raw rooms, fix the per-room randomness, derive superpoints -------------------
    def draw_room(self, xyz, rid):
        """the host-drawn randomness of one tile, a function of (seed, global room id): pick point, shuffle, padding draws"""
        cfg, N = self.cfg, self.cfg.num_points
        self.rng = np.random.default_rng([self.seed, rid])
        n = len(xyz)
        pick = xyz[self.rng.integers(0, n)] + self.rng.normal(0, cfg.noise_init / 10, 3)      # s3dis_dataset.py:119-126
        return dict(n=n, center=np.ascontiguousarray(pick, np.float32),
                    perm=self.rng.permutation(N).astype(np.int32),                             # DP.shuffle_idx :137
                    dup=self.rng.random(N).astype(np.float32))                                 # DP.data_aug's np.random.choice

    def load_rooms(self, rooms, room_ids=None):
        """room_ids: global ids of the rooms (sharded runs); all host-drawn randomness is a function of (seed, id), so a
        sharded run and a single-process run over the union see the same tiles."""
        cfg = self.cfg
        N = cfg.num_points
        self.B = len(rooms)
        self._drop_room_plan()      # the previous rooms' plan, before their arrays go
        self._dist = None           # the sharded run's static tables (labelled mask, sizes, exchange buffers) belong to the loaded rooms
        self.room_ids = list(range(len(rooms))) if room_ids is None else list(room_ids)
        self.rooms = []
        centers, perms, dups = [], [], []
        for (xyz, rgb, lab), rid in zip(rooms, self.room_ids):
            r = self.draw_room(xyz, rid)
            centers.append(r["center"]); perms.append(r["perm"]); dups.append(r["dup"])
            self.rooms.append(r)
        # the rooms of the batch live concatenated in HBM: one batched call per front-end stage
        self.room_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in rooms])]).astype(np.int64)
        nt = int(self.room_off[-1])
        self.raw_p = DevArray.from_host(np.concatenate([r[0] for r in rooms]).astype(np.float32))
        self.raw_c = DevArray.from_host(np.concatenate([r[1] for r in rooms]).astype(np.float32))
        self.raw_l = DevArray.from_host(np.concatenate([r[2] for r in rooms]).astype(np.int32).reshape(-1, 1))
        self.sub_p = DevArray((nt, 3), np.float32); self.sub_c = DevArray((nt, 3), np.float32); self.sub_l = DevArray((nt, 1), np.int32)
        self.sub_m = DevArray((len(rooms) + 1,), np.int64)
        self.centers = np.ascontiguousarray(np.stack(centers), np.float32)
        self.perm = DevArray.from_host(np.stack(perms)); self.dup = DevArray.from_host(np.stack(dups))
        B = self.B
        self.xyz = DevArray((B, N, 3), np.float32); self.feat = DevArray((B, N, 6), np.float32)
        self.tile_l = DevArray((B * N,), np.int32)        # queried_pc_label (s3dis_dataset.py:141): the labelled regions' ground truth
        L, K = cfg.num_layers, cfg.k_n
        self.sizes = [N]
        for ratio in cfg.sub_sampling_ratio:
            self.sizes.append(self.sizes[-1] // ratio)
        self.neigh = [DevArray((B, self.sizes[i], K), np.int32) for i in range(L)]
        self.interp = [DevArray((B, self.sizes[i], 1), np.int32) for i in range(L)]
        self.probs = DevArray((B * N, cfg.num_classes), np.float32); self.f32 = DevArray((B * N, 32), np.float32)
        self.unc = DevArray((B * N,), np.float32); self.cls = DevArray((B * N,), np.int32)
        # superpoints of the (fixed) tiles: computed once from a dry run of the geometric front end.  The dry run also settles which
        # implementation of the batched grid subsample these rooms get: the bucket partition reports a cloud it cannot take (a grid of
        # more than 16384 buckets, a voxel of more than 1024 points) through its status, and the rooms then go through the sort
        self.subsample_method = 1 if os.environ.get("SSDR_SUBSAMPLE_METHOD") == "sort" else 0          # (development: A/B of the two implementations)
        # the rooms stay as uploaded while tiles are drawn from them: what the bucket partition derives from the points alone (bounding boxes, grids, per-bucket
        # counts and offsets) is built once, behind the upload, and every _front_end starts at the bucket order.  SSDR_FE_ROOM_PLAN=0 (development: A/B runs in
        # one build) keeps the call that derives it every time
        if self.subsample_method == 0 and os.environ.get("SSDR_FE_TILE_PRUNE", "1") != "0" and os.environ.get("SSDR_FE_ROOM_PLAN", "1") != "0":
            plan = C.c_void_p()
            _lib.check(_lib.lib().ssdr_rooms_plan_create_dev(self.raw_p.ptr, self.raw_c.ptr, 3, self.raw_l.ptr, 1, _lib.ptr(self.room_off), self.B, cfg.sub_grid_size,
                                                             self.front_stream, C.byref(plan)))
            self._room_plan, self._room_plan_lib = plan.value, _lib.lib()
        self._front_end()
        _lib.sync()
        st = C.c_int32()
        rc = _lib.lib().ssdr_grid_subsample_status(self.front_stream, C.byref(st))
        if rc != 0 and (st.value & 6):
            self.subsample_method = 1
            self._drop_room_plan()          # (the sort has no use for it)
            self._front_end()
            _lib.sync()
            _lib.check(_lib.lib().ssdr_grid_subsample_status(self.front_stream, None))
        else:
            _lib.check(rc)
        tiles = self.xyz.to_host()
        offs, pts, cloud = [np.zeros(1, np.int32)], [], []
        for b in range(B):
            o, p = synthetic.superpoints_from_tile(tiles[b])
            pts.append(p + b * N); offs.append(o[1:] + offs[-1][-1]); cloud.append(np.full(len(o) - 1, b, np.int32))
        labeled = {}
        sp_cloud = np.concatenate(cloud)
        for b in range(B):           # "already labelled" superpoints (stand-in for the regions total_obj["unlabeled"] no longer lists)
            ids = np.flatnonzero(sp_cloud == b)
            rng = np.random.default_rng([self.seed, self.room_ids[b], 1])
            labeled[b] = set(rng.choice(ids, min(self.labeled_per_tile, len(ids)), replace=False).tolist())
        self.n_pts = B * N
        self.pt_off = np.arange(B + 1, dtype=np.int64) * N
        self._set_regions(np.concatenate(offs), np.concatenate(pts), sp_cloud, labeled,
                          np.random.default_rng([self.seed, 999983]).integers(0, cfg.num_classes, 4000))
        return self

    @classmethod
    def from_clouds(cls, clouds, labeled, selected_class_list, config=ConfigS3DIS, room_ids=None, **kw):
        """The scoring + selection half alone, over clouds given with their network outputs (no front end, no network): clouds[b] = dict(xyz [n,3],
        gt [n], probs [n,C], feat [n,32], offsets [S_b+1], points) — what prediction() / compute_features see per cloud (sampler2.py:580-642,
        :313-342); labeled[b] = the regions of cloud b (ids inside the cloud) that total_obj["unlabeled"] no longer lists.  Clouds may differ in
        size: every array is the concatenation, superpoints are one CSR over it.  step_selection() runs the round."""
        n_of = [len(c["xyz"]) for c in clouds]
        p0 = np.concatenate([[0], np.cumsum(n_of)]).astype(np.int64)
        offs, pts, cloud, lab, s0 = [np.zeros(1, np.int64)], [], [], {}, 0
        for b, c in enumerate(clouds):
            o = np.asarray(c["offsets"], np.int64)
            offs.append(o[1:] + offs[-1][-1]); pts.append(np.asarray(c["points"], np.int64) + p0[b]); cloud.append(np.full(len(o) - 1, b, np.int32))
            lab[b] = set(int(s) + s0 for s in labeled[b]); s0 += len(o) - 1
        hp = cls.from_device(DevArray.from_host(np.concatenate([np.asarray(c["xyz"], np.float32) for c in clouds])),
                               DevArray.from_host(np.concatenate([np.asarray(c["probs"], np.float32) for c in clouds])),
                               DevArray.from_host(np.concatenate([np.asarray(c["feat"], np.float32) for c in clouds])),
                               DevArray.from_host(np.concatenate([np.asarray(c["gt"]).astype(np.int32) for c in clouds])),
                               np.concatenate(offs), np.concatenate(pts), np.concatenate(cloud), lab, selected_class_list, config, room_ids=room_ids, **kw)
        hp.pt_off = p0
        return hp

    @classmethod
    def from_device(cls, xyz, probs, f32, labels, sp_off, sp_pts, sp_cloud, labeled, selected_class_list, config=ConfigS3DIS, room_ids=None, **kw):
        """from_clouds over arrays that are already resident (xyz [n,3] f32, probs [n,C] f32, f32 [n,32] f32, labels [n] i32: DevArray or anything
        with .ptr): the superpoints as one CSR over the n points (host arrays), sp_cloud [S] = the cloud of every superpoint (ascending),
        labeled[b] = GLOBAL ids of cloud b's labelled regions.  This is how one AL round ends at the reference's scale (ALRound): the network
        outputs of all clouds stay where the batches' inference left them."""
        hp = cls(None, config, **kw)
        sp_cloud = np.asarray(sp_cloud, np.int32)
        hp.B = int(sp_cloud.max()) + 1 if len(sp_cloud) else 0
        hp._dist = None; hp.room_ids = list(range(hp.B)) if room_ids is None else list(room_ids); hp.rooms = []      # room_ids: the clouds' global ids (sharded runs)
        hp.n_pts = int(xyz.shape[0])
        hp.xyz, hp.probs, hp.f32, hp.tile_l = xyz, probs, f32, labels
        hp.unc = DevArray((hp.n_pts,), np.float32); hp.cls = DevArray((hp.n_pts,), np.int32)
        hp._set_regions(sp_off, sp_pts, sp_cloud, labeled, selected_class_list)
        return hp

    def step_selection(self, comm=None):
        """scoring + selection over the resident network outputs (from_clouds); comm: the sharded run's exchanges"""
        if comm is not None and self.selector == "coregcn":
            raise ValueError('selector="coregcn" with a communicator: the sharded form of the trained-GCN selector is not offered')
        if self.selector in REGION_SAMPLERS:
            return self._region_select(comm)
        self._score_async(comm)
        return self._select(comm)

    def _set_regions(self, sp_off, sp_pts, sp_cloud, labeled, selected_class_list):
        """superpoints (one CSR over the batch's points), which of them are already labelled, the already-selected class list; then everything
        the selection derives from them once: the ranked population, the labelled rows' draw, the device rule's static tables"""
        cfg, B = self.cfg, self.B
        self.sp_off_h = np.asarray(sp_off).astype(np.int32); self.sp_pts_h = np.asarray(sp_pts).astype(np.int32)
        self.sp_cloud_h = np.asarray(sp_cloud).astype(np.int32)
        self.S = len(self.sp_off_h) - 1
        self.sp_base = np.searchsorted(self.sp_cloud_h, np.arange(B)).astype(np.int64).tolist()      # (clouds are ascending: every cloud owns at least one region)
        self.sp_off = DevArray.from_host(self.sp_off_h); self.sp_pts = DevArray.from_host(self.sp_pts_h)
        self.d_sp_cloud = DevArray.from_host(self.sp_cloud_h if self.S else np.zeros(1, np.int32))
        self.region_unc = DevArray((self.S,), np.float64); self.dom = DevArray((self.S,), np.int32); self.dom_cnt = DevArray((self.S,), np.int32)
        self.gt_dom = DevArray((self.S,), np.int32); self.gt_purity = DevArray((self.S,), np.float64)
        self.sorted_inds = DevArray((self.S,), np.int32)
        self._class_list_h = np.asarray(selected_class_list).astype(np.int32).reshape(-1)      # host mirror: label_selected appends to both
        self.selected_class_list = DevArray.from_host(self._class_list_h)
        self.hist = DevArray((64,), np.int32)
        self.sp_size_h = np.diff(self.sp_off_h)
        self.set_labeled(labeled)

    def _room_sp(self, ids):
        """(room id, superpoint inside its room) of local region ids"""
        c = self.sp_cloud_h[ids]
        return np.asarray(self.room_ids, np.int64)[c], ids - np.asarray(self.sp_base, np.int64)[c]

    def set_labeled(self, labeled):
        """labeled[b] = the (global) ids of cloud b's regions that are already labelled (what total_obj["unlabeled"] no longer lists)"""
        cfg = self.cfg
        self._dist = None; self.global_order = None      # a sharded run's static tables (labelled mask, populations, the global draw) belong to the labelling
        self._unl_lists = self._drawn0 = None            # ... and so do the host draws' unlabelled lists and a drawn, not yet labelled iteration
        self.labeled = labeled
        self.labeled_mask = np.zeros(self.S, bool)
        for b in self.labeled:
            self.labeled_mask[list(self.labeled[b])] = True
        # prediction()'s population (sampler2.py:612-631): unlabelled regions of at least min_size points are ranked; labelled ones of at least
        # min_size points are the pool the labelled rows are drawn from; the rest takes no part.  skip_mask = not in the ranked population
        big = self.sp_size_h >= self.min_size
        if self.max_size is not None:
            big &= self.sp_size_h <= self.max_size
        self.skip_mask = self.labeled_mask | ~big
        self.lab_pool = np.flatnonzero(self.labeled_mask & big)                 # cloud by cloud, ascending superpoint id
        # the pool's ground-truth dominant labels from the resident labels (the reference reads them from the cloud's PLY, :283-289)
        _lib.check(_lib.lib().ssdr_dominant_label_dev(self.tile_l.ptr, self.sp_off.ptr, self.sp_pts.ptr, self.S, max(cfg.num_classes, 1), self.gt_dom.ptr,
                                                      self.gt_purity.ptr, self.front_stream))
        _lib.sync(self.front_stream)
        self.lab_pool_dom = self.gt_dom.to_host()[self.lab_pool]
        self._draw_labelled(self.lab_pool, self.lab_pool_dom, np.arange(len(self.lab_pool)))

    def _draw_labelled(self, pool_sp, pool_dom_all, mine):
        """get_labeled_selection_cloudname_spidx_pointidx's draw (sampler2.py:294-302) over the pool given by its dominant labels `pool_dom_all` (all
        ranks' pools in cloud order for a sharded run; `mine` = this process's positions in it, pool_sp = their local superpoint ids)."""
        drawn = sampler.get_labeled_selection(pool_dom_all, self.cfg.num_classes, self.round_num, np.random.RandomState(self.label_seed))
        keep = np.zeros(len(pool_dom_all), bool); keep[drawn] = True
        rows = np.asarray(pool_sp, np.int64)[keep[np.asarray(mine, np.int64)]]
        self.lab_rows = {b: sorted(int(x) for x in rows[self.sp_cloud_h[rows] == b]) for b in range(self.B)}      # cloud ascending, superpoint ascending
        self._select_static()

    def _select_static(self):
        """Static tables and capacities of the device-side candidate rule (ssdr_gcn_fps_sampling_dev): which regions are labelled, where a
        cloud's superpoints start, its labelled regions, and upper bounds of what the rule can produce (the counts themselves are the
        ranking's and stay on the device)."""
        B, S = self.B, self.S
        base = np.concatenate([np.asarray(self.sp_base, np.int64), [S]])
        lab = [self.lab_rows.get(b, []) for b in range(B)]
        lab_off = np.concatenate([[0], np.cumsum([len(l) for l in lab])]).astype(np.int32)
        lab_sp = np.array([s for l in lab for s in l] + [0], np.int32)
        nvalid = np.array([int((~self.skip_mask[base[b]:base[b + 1]]).sum()) for b in range(B)], np.int64)
        nlab = np.diff(lab_off).astype(np.int64)
        batch = self.batch_size if self.batch_size is not None else self.select_per_tile * B      # sampling()'s batch_size
        picks, cap_unl, _, cap_rows, cap_nmax, cap_sq = _capacities(nvalid, nlab, batch)
        region = {}
        if self.selector == "edcd":      # the edcd round's rows are the candidates alone (the branch draws no labelled rows)
            _, _, _, _, e_nmax, e_sq = _capacities(nvalid, np.zeros_like(nvalid), batch)
            region = dict(e_cap_nmax=e_nmax, e_cap_sq=e_sq)
        elif self.selector == "topk":
            region = dict(d_topk=DevArray((RES_HEADER + max(min(batch, S), 1),), np.int32))
        self._sel_static = dict(region,
            lab_cloud=np.repeat(np.arange(B, dtype=np.int64), nlab), lab_sp_h=lab_sp[:-1].astype(np.int64),
            d_lab=DevArray.from_host(self.skip_mask.astype(np.uint8)), d_base=DevArray.from_host(base.astype(np.int32)),
            d_lab_off=DevArray.from_host(lab_off), d_lab_sp=DevArray.from_host(lab_sp), n_lab=int(nlab.sum()), batch=batch, picks=picks, cap_unl=cap_unl,
            cap_rows=cap_rows, cap_nmax=cap_nmax, cap_sq=cap_sq, d_result=DevArray((RES_HEADER + picks + cap_rows,), np.int32))

    # ---- stages ------------------------------------------------------------------------------------------------
    def _front_end(self):
        """grid-subsample + tile of every room of the batch, one batched launch sequence per stage (on front_stream)."""
        cfg, L = self.cfg, _lib.lib()
        st = self.front_stream
        _lib.check(L.ssdr_grid_subsample_set_method(self.subsample_method))
        # the bucket partition reduces only the buckets the tiles' rows can lie in (sub_* / sub_m then hold those rows); SSDR_FE_TILE_PRUNE=0 (development:
        # A/B runs) and the sort keep the two calls
        if self.subsample_method == 0 and os.environ.get("SSDR_FE_TILE_PRUNE", "1") != "0":
            if self._room_plan is not None and os.environ.get("SSDR_FE_ROOM_PLAN", "1") != "0":
                _lib.check(L.ssdr_tile_from_rooms_planned_batch_dev(self._room_plan, self.raw_p.ptr, self.raw_c.ptr, 3, self.raw_l.ptr, 1, _lib.ptr(self.room_off), self.B,
                                                                    cfg.sub_grid_size, self.sub_p.ptr, self.sub_c.ptr, self.sub_l.ptr, self.sub_m.ptr, _lib.ptr(self.centers),
                                                                    cfg.num_points, self.perm.ptr, self.dup.ptr, 1.0 / 255.0, self.xyz.ptr, self.feat.ptr, None, self.tile_l.ptr, st))
                return
            _lib.check(L.ssdr_tile_from_rooms_batch_dev(self.raw_p.ptr, self.raw_c.ptr, 3, self.raw_l.ptr, 1, _lib.ptr(self.room_off), self.B, cfg.sub_grid_size,
                                                        self.sub_p.ptr, self.sub_c.ptr, self.sub_l.ptr, self.sub_m.ptr, _lib.ptr(self.centers), cfg.num_points,
                                                        self.perm.ptr, self.dup.ptr, 1.0 / 255.0, self.xyz.ptr, self.feat.ptr, None, self.tile_l.ptr, st))
            return
        _lib.check(L.ssdr_grid_subsample_batch_dev(self.raw_p.ptr, self.raw_c.ptr, 3, self.raw_l.ptr, 1, _lib.ptr(self.room_off), self.B, cfg.sub_grid_size,
                                                   self.sub_p.ptr, self.sub_c.ptr, self.sub_l.ptr, self.sub_m.ptr, st))
        _lib.check(L.ssdr_tile_select_batch_dev(self.sub_p.ptr, self.sub_c.ptr, 3, self.sub_m.ptr, _lib.ptr(self.room_off), self.B, _lib.ptr(self.centers),
                                                cfg.num_points, self.perm.ptr, self.dup.ptr, 1.0 / 255.0, self.xyz.ptr, self.feat.ptr, None, self.sub_l.ptr, self.tile_l.ptr, st))

    def _pyramid(self):
        cfg = self.cfg
        arr = C.c_void_p * cfg.num_layers
        r = np.asarray(cfg.sub_sampling_ratio, np.int32)
        _lib.check(_lib.lib().ssdr_knn_pyramid_dev(self.xyz.ptr, self.B, cfg.num_points, cfg.num_layers, _lib.ptr(r), cfg.k_n,
                                                   arr(*[a.ptr for a in self.neigh]), None, arr(*[a.ptr for a in self.interp]),
                                                   self.knn_stream if self.knn_stream is not None else self.stream))

    def _infer(self):
        self.net.infer_dev(self.B, self.cfg.num_points, self.feat.ptr, self.xyz.ptr, [a.ptr for a in self.neigh], [a.ptr for a in self.interp],
                           self.probs.ptr, self.f32.ptr, self.stream)

    def _dist_setup(self, comm):
        """Static tables of the sharded run, exchanged once (untimed): every rank's superpoint count, labelled mask, cloud and room ids.
        Global superpoint id = rank * Smax + local id (the all-gather of exchange 2 is padded to Smax rows per rank)."""
        if self._dist is not None and self._dist["comm"] is comm:
            return self._dist
        W = comm.world
        # the labelled rows are drawn from the pool of ALL ranks at once (sampler2.py:294-302 draws over every cloud's labelled regions): exchange the
        # pools' ground-truth dominant labels, order them as one process over the union would meet them (room id, superpoint), draw, keep one's own
        npool = comm.allgather_host(np.array([len(self.lab_pool)], np.int64)).reshape(-1)
        Pmax = max(int(npool.max()), 1)
        def padp(a):
            out = np.full(Pmax, -1, np.int64); out[: len(a)] = a; return out
        pool_room, pool_sp = self._room_sp(self.lab_pool)
        g_room = comm.allgather_host(padp(pool_room)).reshape(-1)
        g_sp = comm.allgather_host(padp(pool_sp)).reshape(-1)
        g_dom = comm.allgather_host(padp(self.lab_pool_dom)).reshape(-1)
        g_rank = np.repeat(np.arange(W), Pmax); g_loc = np.tile(np.arange(Pmax), W)
        live = np.flatnonzero(g_room >= 0)
        live = live[np.lexsort((g_sp[live], g_room[live]))]
        pos_of = np.full(Pmax, -1, np.int64)
        me = g_rank[live] == comm.rank
        pos_of[g_loc[live][me]] = np.flatnonzero(me)
        self._draw_labelled(self.lab_pool, g_dom[live], pos_of[: len(self.lab_pool)])
        S_all = comm.allgather_host(np.array([self.S, self.B], np.int64))
        Smax = int(S_all[:, 0].max())
        def padded(a, fill):
            out = np.full(Smax, fill, np.int64); out[: self.S] = a; return out
        lab = comm.allgather_host(padded(self.skip_mask.astype(np.int64), 1)).reshape(-1)          # not in the ranked population (labelled / below min_size); padding counts as such
        cloud = comm.allgather_host(padded(self.sp_cloud_h, -1))                                      # local cloud index
        my_room, my_spin = self._room_sp(np.arange(self.S))
        room = comm.allgather_host(padded(my_room, -1)).reshape(-1)
        spin = comm.allgather_host(padded(my_spin, -1)).reshape(-1)
        Bmax = int(S_all[:, 1].max())
        gcloud = (cloud + (np.arange(W)[:, None] * Bmax)).reshape(-1)                                 # global cloud index, rank-major
        gcloud[cloud.reshape(-1) < 0] = -1
        # sampling()'s batch_size is ONE number for the whole round (ssdr_main_S3DIS2.py:134: 10 000 regions whatever the number of clouds): with
        # batch_size set it stays that, however many ranks share the clouds; the default grows it with the tiles (select_per_tile each)
        batch = self.batch_size if self.batch_size is not None else self.select_per_tile * int(S_all[:, 1].sum())
        # the device-side rule of the sharded run (ssdr_gcn_fps_sharded_local_dev): global labelled mask (padding = labelled), where every global cloud's
        # regions start, and the capacities the static tables bound
        base_l = np.concatenate([np.asarray(self.sp_base, np.int64), np.full(Bmax + 1 - self.B, self.S, np.int64)])      # local, padded to Bmax + 1 entries
        gbase = (comm.allgather_host(base_l[:Bmax]) + np.arange(W)[:, None] * Smax).reshape(-1)
        gbase = np.concatenate([gbase, [W * Smax]]).astype(np.int32)
        nvalid_c = np.array([int((~self.skip_mask[base_l[b]:base_l[b + 1]]).sum()) for b in range(self.B)], np.int64)
        nvalid_all = comm.allgather_host(np.array([int(nvalid_c.sum())], np.int64)).reshape(-1)
        picks = int(min(batch, nvalid_all.sum()))
        T = self._sel_static
        nlab_c = np.diff(T["d_lab_off"].to_host()).astype(np.int64)
        # this rank's bounds under the GLOBAL number of picks (where its own clouds hold fewer regions than that, they offer all they have either way)
        _, _, _, cap_rows, cap_nmax, cap_sq = _capacities(nvalid_c, nlab_c, picks)
        nu_dev = max(int(np.minimum(2 * picks, nvalid_all).max()), 1)
        rep = max(int(os.environ.get("SSDR_EMULATE_WORLD", "1")), 1)       # development: the FPS load of `rep` x the ranks (tools/gpu_emulate_world.sh)
        cap_fps = max(rep * int(min(2 * picks, nvalid_all.sum())), 1)
        nlab = comm.allgather_host(np.array([int(T["n_lab"])], np.int64)).reshape(-1)
        # the k-center selector also sends every rank's labelled regions' rows (behind its candidates, padded to nl_max) and seeds the global chain with them
        kc = self.selector == "kcenter"
        nl_max = int(nlab.max()) if kc else 0
        n_lab_all = int(nlab.sum()) if kc else 0
        per = nu_dev + nl_max
        dev = dict(picks=picks, cap_rows=cap_rows, cap_nmax=cap_nmax, cap_sq=cap_sq, nu_max=nu_dev,
                   cap_fps=cap_fps, rep=rep, d_glab=DevArray.from_host((lab != 0).astype(np.uint8)), d_gbase=DevArray.from_host(gbase),
                   nl_max=nl_max, n_lab_all=n_lab_all, per=per,
                   d_send=DevArray((per, 32), np.float64), d_gath=DevArray((W, per, 32), np.float64), d_glob=DevArray((cap_fps + n_lab_all + 1, 32), np.float64),
                   d_nlab_off=DevArray.from_host(np.concatenate([[0], np.cumsum(nlab)]).astype(np.int32)), d_already=DevArray((max(n_lab_all, 1),), np.int32),
                   d_plan=DevArray((_plan_gcand(W, nu_dev) + W * nu_dev,), np.int32), d_out=DevArray((max(rep * picks, 1),), np.int32))
        if self.selector == "edcd":      # this rank's share of the edcd round: its own candidates and picks, no labelled rows
            own, _, _, e_rows, e_nmax, e_sq = _capacities(nvalid_c, np.zeros_like(nvalid_c), batch)
            dev.update(e_picks=own, e_cap_rows=e_rows, e_cap_nmax=e_nmax, e_cap_sq=e_sq, e_result=DevArray((RES_HEADER + own + e_rows,), np.int32))
        elif self.selector == "topk":
            dev.update(t_result=DevArray((RES_HEADER + max(min(batch, self.S), 1),), np.int32))
        self._dist = dict(dev=dev, comm=comm, Smax=Smax, Bmax=Bmax, valid=lab == 0, gcloud=gcloud, room=room, spin=spin, batch=batch,
                          S_total=int(S_all[:, 0].sum()), n_pop=int(nvalid_all.sum()), nu_max=int(min(2 * batch, Smax)),
                          nlab=nlab, nvalid_all=nvalid_all, d_gcloud=DevArray.from_host(gcloud.astype(np.int32)),      # (the sharded labelling: every global region's global cloud)
                          d_lab=DevArray.from_host(self.skip_mask.astype(np.uint8)),
                          d_masked=DevArray((Smax,), np.float64), d_all=DevArray((W * Smax,), np.float64), d_ord=DevArray((W * Smax,), np.int32))
        return self._dist

    def _score_async(self, comm=None):
        """The scoring stage, enqueued, never waits.  With a communicator the two exchanges run on the same stream, on device buffers:
        all-reduce of the class histogram, all-gather of the (masked, padded) region uncertainties, then the global ranking."""
        cfg, L = self.cfg, _lib.lib()
        n = self.n_pts
        self._pred_resident = True
        um = {"lc": 0, "entropy": 1, "sb": 2}[[a for a in self.sampler_args if a in ("lc", "entropy", "sb")][0]]
        rm = {"mean": 0, "sum_weight": 1, "WetSU": 2}[[a for a in self.sampler_args if a in ("mean", "sum_weight", "WetSU")][0]]
        st = self.score_stream if self.score_stream is not None else self.stream
        _lib.check(L.ssdr_point_uncertainty_dev(self.probs.ptr, n, cfg.num_classes, um, self.unc.ptr, self.cls.ptr, st))
        _lib.check(L.ssdr_region_stats_dev(self.unc.ptr, self.cls.ptr, self.sp_off.ptr, self.sp_pts.ptr, self.S, cfg.num_classes, rm,
                                           self.region_unc.ptr, self.dom.ptr, self.dom_cnt.ptr, st))
        # the labelled regions' dominant GROUND-TRUTH class (their dominant_point_ids, sampler2.py:288-291) from this batch's tile labels
        _lib.check(L.ssdr_dominant_label_dev(self.tile_l.ptr, self.sp_off.ptr, self.sp_pts.ptr, self.S, max(cfg.num_classes, 1), self.gt_dom.ptr, self.gt_purity.ptr, st))
        # class balance over the ranked population only (prediction() appends only unlabelled regions to region_class, :612-627): "classbal"
        # (add_classbal, :256-260) is the same without the already-selected list and is tested first, as the reference does (:635-638)
        bal = "classbal" in self.sampler_args or "clsbal" in self.sampler_args
        nsel = 0 if "classbal" in self.sampler_args else self.selected_class_list.shape[0]
        T = self._sel_static
        if comm is None:
            if bal:
                _lib.check(L.ssdr_clsbal_dev(self.dom.ptr, self.S, T["d_lab"].ptr, self.selected_class_list.ptr, nsel, self.region_unc.ptr, st))
            _lib.check(L.ssdr_rank_regions_dev(self.region_unc.ptr, self.S, self.sorted_inds.ptr, st))
            self.global_order = None
            return
        D = self._dist_setup(comm)
        if bal:       # exchange 1: the class histogram is global (the already-selected list is counted once, on rank 0)
            _lib.check(L.ssdr_class_hist_dev(self.dom.ptr, self.S, D["d_lab"].ptr, self.selected_class_list.ptr, nsel if comm.rank == 0 else 0, self.hist.ptr, st))
            comm.allreduce_sum_(self.hist, st)
            _lib.check(L.ssdr_clsbal_hist_dev(self.dom.ptr, self.S, self.hist.ptr, D["n_pop"] + nsel, self.region_unc.ptr, st))
        # exchange 2: rank the regions of ALL ranks; labelled regions (and the padding) are -inf and sort last
        _lib.check(L.ssdr_mask_regions_dev(self.region_unc.ptr, D["d_lab"].ptr, self.S, D["Smax"], D["d_masked"].ptr, st))
        comm.allgather_(D["d_masked"], D["d_all"], st)
        _lib.check(L.ssdr_rank_regions_dev(D["d_all"].ptr, comm.world * D["Smax"], D["d_ord"].ptr, st))
        self.global_order = D

    def _candidates(self, order, valid, cloud, batch_size):
        """create_file_top_and_all + the candidate rule of sampling() (sampler2.py:533-552, :745-753) on index lists: `order` ranks
        the regions by descending uncertainty, valid[i] = region i may compete (not labelled), cloud[i] = its cloud.  Returns the
        candidates (cloud ascending, descending uncertainty inside a cloud) and their clouds, the number to select, and selected_num per cloud.
        The order is canonical: the reference's own depends on a shuffled DataLoader (sampler2.py:323) and carries no meaning."""
        order = np.asarray(order, np.int64)
        cand = order[valid[order]]                            # labelled regions never compete
        c = cloud[cand]
        nc = int(cloud.max()) + 1 if len(cloud) else 0
        ntop = np.bincount(c[: min(batch_size, len(order))], minlength=nc)      # selected_num per cloud (len(file_list_top[cloud])): the first batch_size candidates are "top"
        # cloud ascending, descending uncertainty inside a cloud (a stable sort of 16-bit keys is a radix sort in NumPy: the sharded run ranks
        # the regions of ALL ranks here, 8 x as many on 8 GPUs)
        grp = np.argsort(c.astype(np.uint16) if nc <= 65536 else c, kind="stable")
        cand, c = cand[grp], c[grp]
        counts = np.bincount(c, minlength=nc)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if nc else np.zeros(0, np.int64)
        pos = np.arange(len(cand)) - first[c]
        take = pos < 2 * ntop[c]                              # candidates = first 2 x selected_num of the cloud (:748)
        return cand[take], c[take], int(ntop.sum()), ntop

    def _select(self, comm=None):
        self._select_issue(comm)
        return self._select_collect()

    def _select_issue(self, comm=None):
        """Everything of the selection up to the enqueued FPS chain, by route: the device routes decide nothing on the host and upload nothing; the host
        route (SSDR_SELECT_HOST_RULE, a round without picks, k-center without a labelled row) does both here.  Leaves the _Issued record in _pending."""
        if self.selector in ("edcd", "topk"):
            self._pending = self._select_issue_region(comm)
            return
        _lib.check(_lib.lib().ssdr_select_set_chamfer_mode(self.chamfer_mode))
        T, D, kc = self._sel_static, self.global_order, self.selector == "kcenter"
        if self.selector == "coregcn":
            route, path = self._issue_coregcn, "device"
        elif D is None and T["picks"] > 0 and (not kc or T["n_lab"] > 0) and not _host_rule():
            route, path = self._issue_device, "device"
        elif D is not None and D["dev"]["picks"] > 0 and (not kc or D["dev"]["n_lab_all"] > 0) and not _host_rule():
            route, path = self._issue_sharded, "sharded-device"
        else:
            route, path = self._issue_host, "host"
        self.rule_path = path
        self._pending = route(comm)

    def _issue_coregcn(self, comm):
        L, st, T = _lib.lib(), self.sel_stream, self._sel_static
        if comm is not None or self.global_order is not None:
            raise ValueError('selector="coregcn" with a communicator: the sharded form of the trained-GCN selector is not offered')
        if T["n_lab"] == 0:
            raise ValueError("GCN_sampling: no labelled row: the loss is a mean over an empty set (gcn.py:81-83)")
        rec = _Issued("device", None, T["d_result"], T["picks"])
        d_init = DevArray.from_host(sampler.gcn_init_params(self.gcn_seed), st); rec.keep.append(d_init)
        _lib.check(L.ssdr_gcn_sampling_dev(self.f32.ptr, 32, self.cls.ptr, self.dom.ptr, self.tile_l.ptr, self.gt_dom.ptr, self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr,
                                           self.sorted_inds.ptr, self.S, T["d_lab"].ptr, T["d_base"].ptr, self.B, T["d_lab_off"].ptr, T["d_lab_sp"].ptr,
                                           T["n_lab"], T["batch"], d_init.ptr, self.gcn_steps, self.gcn_dropout, 1e-3, 5e-4, 1.2,
                                           self.gcn_seed & 0xffffffffffffffff, sampler.GCN_FORMS[self.gcn_form], T["cap_rows"], T["cap_nmax"], T["cap_sq"],
                                           T["cap_unl"], T["picks"], T["d_result"].ptr, st))
        return rec

    def _issue_device(self, comm):
        """candidate rule + GCN_FPS_sampling enqueued as one chain: the host decides nothing and uploads nothing (the result is read in _select_collect)"""
        L, st, T = _lib.lib(), self.sel_stream, self._sel_static          # st None: the library stream; a stream of its own lets the selections of consecutive batches overlap
        _lib.check(L.ssdr_gcn_fps_sampling_dev(self.f32.ptr, 32, self.cls.ptr, self.dom.ptr, self.tile_l.ptr, self.gt_dom.ptr, self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr,
                                               self.sorted_inds.ptr, self.S, T["d_lab"].ptr, T["d_base"].ptr, self.B, T["d_lab_off"].ptr, T["d_lab_sp"].ptr,
                                               T["n_lab"], T["batch"], int(self.gcn_number), int(self.gcn_top), 1 if self.selector == "kcenter" else 0, int(self.fps_start),
                                               T["cap_rows"], T["cap_nmax"], T["cap_sq"], T["cap_unl"], T["picks"], T["d_result"].ptr, st))
        return _Issued("device", comm, T["d_result"], T["picks"])

    def _issue_sharded(self, comm):
        """the sharded run, still without a host decision: the rule over the global ranking + this rank's graph, the all-gather of the candidates'
        propagated features (exchange 3), the replicated global FPS — three enqueues, nothing read back here"""
        L, st, T, kc = _lib.lib(), self.sel_stream, self._sel_static, self.selector == "kcenter"
        D = self.global_order; V = D["dev"]
        _lib.check(L.ssdr_gcn_fps_sharded_local_dev(self.f32.ptr, 32, self.cls.ptr, self.dom.ptr, self.tile_l.ptr, self.gt_dom.ptr, self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr,
                                                    T["d_lab_off"].ptr, T["d_lab_sp"].ptr, T["n_lab"], self.B, D["d_ord"].ptr, comm.world * D["Smax"],
                                                    V["d_glab"].ptr, V["d_gbase"].ptr, comm.rank, comm.world, D["Smax"], D["Bmax"], D["batch"],
                                                    int(self.gcn_number), int(self.gcn_top), V["cap_rows"], V["cap_nmax"], V["cap_sq"], V["nu_max"], V["nl_max"],
                                                    V["d_send"].ptr, V["d_plan"].ptr, st))
        comm.allgather_(V["d_send"], V["d_gath"], st)
        if kc:       # BASELINE configuration 4: [candidates | labelled regions] of all ranks, the labelled ones already selected
            _lib.check(L.ssdr_kcenter_gathered_dev(V["d_gath"].ptr, V["d_plan"].ptr, comm.world, V["nu_max"], V["nl_max"], V["d_nlab_off"].ptr, V["n_lab_all"],
                                                   V["cap_fps"] + V["n_lab_all"] + 1, V["picks"], V["d_glob"].ptr, V["d_already"].ptr, V["d_out"].ptr, st))
        else:
            _lib.check(L.ssdr_fps_gathered_dev(V["d_gath"].ptr, V["d_plan"].ptr, comm.world, V["nu_max"], V["cap_fps"], V["rep"], int(self.fps_start), V["rep"] * V["picks"],
                                               V["d_glob"].ptr, V["d_out"].ptr, st))
        rec = _Issued("sharded", comm, V["d_plan"], V["picks"])
        rec.picks = V["d_out"]
        return rec

    def _issue_host(self, comm):
        """The candidate rule on the host, then the batched graph, the propagation and the FPS / k-center chain enqueued over uploaded index tables."""
        L, st, T, D, kc = _lib.lib(), self.sel_stream, self._sel_static, self.global_order, self.selector == "kcenter"
        rec = _Issued("host", comm)
        if D is None:          # (the D2H below runs on the selection stream, which already waits for the scoring stream's work)
            cand, ccloud, sampling_batch, _ = self._candidates(self.sorted_inds.to_host(st), ~self.skip_mask, self.sp_cloud_h, T["batch"])
            unl_c, unl_s = np.asarray(ccloud, np.int64), np.asarray(cand, np.int64)
            rec.rooms, rec.spin = self._room_sp(unl_s)
            counts_r = None
        else:       # every rank derives the global candidate list from the global ranking, then keeps its own rows
            gcand, gcloud, sampling_batch, _ = self._candidates(D["d_ord"].to_host(st), D["valid"], D["gcloud"], D["batch"])
            rec.gcand = gcand                                    # (label_selected(comm=): the picks index this list)
            r_of = gcand // D["Smax"]
            counts_r = np.bincount(r_of, minlength=comm.world)
            mine = r_of == comm.rank
            unl_c, unl_s = (gcloud[mine] - comm.rank * D["Bmax"]).astype(np.int64), (gcand[mine] - comm.rank * D["Smax"]).astype(np.int64)
            rec.rooms, rec.spin = D["room"][gcand], D["spin"][gcand]
        rec.pairs = unl = _Pairs(unl_c, unl_s)                    # (cloud, superpoint) of this rank's candidates
        if sampling_batch == 0:      # nothing to select anywhere (the global count: every rank of a sharded run returns here, before any exchange)
            rec.picks = np.zeros(0, np.int32)
            return rec
        keep = rec.keep
        lab_c, lab_s = T["lab_cloud"], T["lab_sp_h"]              # the labelled regions, cloud by cloud, ascending superpoint id (static)
        sel = np.concatenate([unl_s, lab_s]).astype(np.int32)
        # every cloud's chamfer graph and propagation hop in one batched call (rows grouped cloud by cloud)
        ref_cloud = np.concatenate([unl_c, lab_c])
        order = np.argsort(ref_cloud, kind="stable").astype(np.int32)
        clouds, counts = np.unique(ref_cloud, return_counts=True)
        counts = counts.astype(np.int64)
        coff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        boff = np.concatenate([[0], np.cumsum(counts * counts)]).astype(np.int64)
        ntot, nmax, nsq = int(coff[-1]), int(counts.max()), int(boff[-1])
        n_unl = len(unl_s)
        src = np.zeros(0, np.int32)
        if counts_r is not None:     # exchange 3 is padded to nu_max rows per rank: positions of the real rows in the gathered array
            src = np.concatenate([r * D["nu_max"] + np.arange(c) for r, c in enumerate(counts_r)]).astype(np.int32)
        # ONE upload for all the small index tables (each separate copy is a host round trip behind the kernels in flight)
        parts = [sel, sel[order], order, coff, boff.view(np.int32), src]
        offs = np.cumsum([0] + [(len(p) + 3) // 4 * 4 for p in parts])           # 16-byte aligned pieces
        pack = np.zeros(offs[-1], np.int32)
        for p, o in zip(parts, offs):
            pack[o:o + len(p)] = p
        d_pack = DevArray.from_host(pack, st)
        d_sel, d_gsel, d_rows, d_coff, d_boff, d_src = (d_pack.ptr + 4 * int(o) for o in offs[:-1])
        rows = max(len(sel), D["nu_max"] if counts_r is not None else 0)
        d_mf = DevArray((len(sel), 32), np.float32)
        d_v = DevArray((len(sel), 32), np.float64); d_comb = DevArray((rows, 32), np.float64)
        d_tmp = [DevArray(d_v.shape, np.float64), DevArray(d_v.shape, np.float64)]
        # compute_features (sampler2.py:333, :339): the candidates' members by the predicted classes, the labelled regions' by the ground truth (:288-291)
        if n_unl:
            _lib.check(L.ssdr_segment_mean_features_dev(self.f32.ptr, 32, self.cls.ptr, self.dom.ptr, self.sp_off.ptr, self.sp_pts.ptr, d_sel, n_unl, d_mf.ptr, st))
        if len(sel) > n_unl:
            _lib.check(L.ssdr_segment_mean_features_dev(self.f32.ptr, 32, self.tile_l.ptr, self.gt_dom.ptr, self.sp_off.ptr, self.sp_pts.ptr, d_sel + 4 * n_unl,
                                                        len(sel) - n_unl, d_mf.ptr + 4 * 32 * n_unl, st))
        # float32 -> float64 as np.concatenate / np.matmul promote it (V and the running sum comb start as the same values)
        _lib.check(L.ssdr_widen_f32_f64_dev(d_mf.ptr, len(sel) * 32, d_v.ptr, d_comb.ptr, st))
        d_cen = DevArray((ntot, 3), np.float64); d_dir = DevArray((nsq,), np.float64); d_adj = DevArray((nsq,), np.float64)
        _lib.check(L.ssdr_cloud_graph_batch_dev(self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr, d_gsel, d_coff, d_boff, len(clouds), ntot, nmax,
                                                int(self.gcn_top), d_cen.ptr, d_dir.ptr, d_adj.ptr, st))
        src_v = d_v
        for hop in range(int(self.gcn_number)):
            dst = d_tmp[hop & 1]
            _lib.check(L.ssdr_propagate_batch_dev(d_adj.ptr, d_coff, d_boff, len(clouds), nmax, d_rows, src_v.ptr, 32, dst.ptr, d_comb.ptr, st))
            src_v = dst
        keep += [d_pack, d_cen, d_dir, d_adj, d_v, d_tmp, d_mf, d_comb]
        n_lab = len(lab_s)
        if comm is not None:                                 # exchange 3: the candidates' propagated features, on the selection stream
            nl_max = int(D["nlab"].max()) if kc else 0       # k-center also needs the labelled regions' rows of every rank
            per = D["nu_max"] + nl_max
            d_send = d_comb
            if kc:                                           # [candidates, padded to nu_max | labelled, padded to nl_max]
                send_idx = np.zeros(per, np.int32)
                send_idx[: len(unl)] = np.arange(len(unl)); send_idx[D["nu_max"]: D["nu_max"] + n_lab] = len(unl) + np.arange(n_lab)
                d_sidx = DevArray.from_host(send_idx, st); d_send = DevArray((per, 32), np.float64)
                _lib.check(L.ssdr_gather_rows_dev(d_comb.ptr, d_sidx.ptr, per, 32 * 8, d_send.ptr, st))
                keep += [d_sidx, d_send]
                src = np.concatenate([r * per + np.arange(c) for r, c in enumerate(counts_r)] +
                                     [r * per + D["nu_max"] + np.arange(c) for r, c in enumerate(D["nlab"])]).astype(np.int32)
                d_src_a = DevArray.from_host(src, st); d_src = d_src_a.ptr; keep.append(d_src_a)
                n_lab = int(D["nlab"].sum())
            d_gath = DevArray((comm.world, per, 32), np.float64)
            comm.allgather_(_Prefix(d_send, per * 32), d_gath, st)
            n_unl = int(counts_r.sum())
            n_rows = n_unl + (n_lab if kc else 0)
            d_glob = DevArray((max(n_rows, 1), 32), np.float64)
            _lib.check(L.ssdr_gather_rows_dev(d_gath.ptr, d_src, n_rows, 32 * 8, d_glob.ptr, st))
            keep += [d_gath, d_glob]
            d_comb = d_glob
            rec.comb, rec.comb_n = d_glob, n_rows
        emu = int(os.environ.get("SSDR_EMULATE_WORLD", "0"))
        if emu > 1 and comm is not None and self.selector != "kcenter":
            # development: the FPS LOAD of `emu` ranks on one GPU (the replicated global chain is N^2: N x the rows, N x the picks) — the rows are
            # repeated, the picks beyond the real ones are ties; only the timing means anything (tools/gpu_emulate_world.sh)
            idx = np.tile(np.arange(n_unl, dtype=np.int32), emu)
            d_idx = DevArray.from_host(idx, st); d_big = DevArray((emu * n_unl, 32), np.float64)
            _lib.check(L.ssdr_gather_rows_dev(d_comb.ptr, d_idx.ptr, emu * n_unl, 32 * 8, d_big.ptr, st))
            keep += [d_idx, d_big]
            d_comb, n_unl, sampling_batch = d_big, emu * n_unl, emu * sampling_batch
            rec.emu_mod = len(idx) // emu
        rec.picks = d_out = DevArray((sampling_batch,), np.int32)
        if self.selector == "kcenter":
            d_already = DevArray.from_host((n_unl + np.arange(n_lab)).astype(np.int32), st); keep.append(d_already)
            _lib.check(L.ssdr_kcenter_dev(d_comb.ptr, n_unl + n_lab, 32, d_already.ptr, n_lab, sampling_batch, d_out.ptr, st))
        else:
            _lib.check(L.ssdr_fps_dev(d_comb.ptr, n_unl, 32, int(self.fps_start), sampling_batch, d_out.ptr, st))
        return rec

    def _select_issue_region(self, comm=None):
        """_select_issue of the "edcd" and "topk" selectors; returns the _Issued record.  Device rule (default): one enqueue-only call over the ranking,
        single-process or sharded, nothing read back here.  SSDR_SELECT_HOST_RULE: the candidate rule / the top on the host, then (edcd) the batched graph
        and the batched FPS.  (sel, unl) keep their contract: edcd's unl = the candidate list (cloud ascending, descending uncertainty inside a cloud) and
        sel indexes it; topk's unl = the top regions in rank order and sel = arange.  A sharded rank returns its own clouds' share."""
        if _host_rule():
            route, path = self._issue_region_host, "host"
        elif self.global_order is None:
            route, path = self._issue_region_device, "device"
        else:
            route, path = self._issue_region_sharded, "sharded-device"
        self.rule_path = path
        return route(comm)

    def _issue_region_device(self, comm):
        L, st, T = _lib.lib(), self.sel_stream, self._sel_static
        if self.selector == "edcd":
            _lib.check(L.ssdr_edcd_sampling_dev(self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr, self.sorted_inds.ptr, self.S, T["d_lab"].ptr, T["d_base"].ptr, self.B,
                                                T["batch"], T["cap_unl"], T["e_cap_nmax"], T["e_cap_sq"], T["picks"], T["d_result"].ptr, st))
            return _Issued("device", comm, T["d_result"], T["picks"])
        _lib.check(L.ssdr_topk_regions_dev(self.sorted_inds.ptr, self.S, T["d_lab"].ptr, T["batch"], 0, self.S, T["d_topk"].ptr, T["d_topk"].ptr + 4 * RES_HEADER, st))
        return _Issued("topk", comm, T["d_topk"], int(T["d_topk"].shape[0]) - RES_HEADER)

    def _issue_region_sharded(self, comm):
        L, st, D = _lib.lib(), self.sel_stream, self.global_order
        V = D["dev"]; lo = comm.rank * D["Smax"]
        if self.selector == "edcd":
            _lib.check(L.ssdr_edcd_sampling_sharded_dev(self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr, self.B, D["d_ord"].ptr, comm.world * D["Smax"], V["d_glab"].ptr,
                                                        V["d_gbase"].ptr, comm.rank, comm.world, D["Smax"], D["Bmax"], D["batch"], V["e_cap_rows"], V["e_cap_nmax"],
                                                        V["e_cap_sq"], V["e_picks"], V["e_result"].ptr, st))
            return _Issued("device", comm, V["e_result"], V["e_picks"])
        _lib.check(L.ssdr_topk_regions_dev(D["d_ord"].ptr, comm.world * D["Smax"], V["d_glab"].ptr, D["batch"], lo, lo + self.S, V["t_result"].ptr,
                                           V["t_result"].ptr + 4 * RES_HEADER, st))
        return _Issued("topk", comm, V["t_result"], int(V["t_result"].shape[0]) - RES_HEADER)

    def _issue_region_host(self, comm):
        L, st, T, D = _lib.lib(), self.sel_stream, self._sel_static, self.global_order
        rec = _Issued("host", comm)
        if D is None:
            order, valid, cloud, batch, sub_c, sub_s = self.sorted_inds.to_host(st), ~self.skip_mask, self.sp_cloud_h, T["batch"], 0, 0
            room, spin = self._room_sp(np.arange(self.S))
        else:
            order, valid, cloud, batch, sub_c, sub_s = D["d_ord"].to_host(st), D["valid"], D["gcloud"], D["batch"], comm.rank * D["Bmax"], comm.rank * D["Smax"]
            room, spin = D["room"], D["spin"]
        rec.gorder = order = np.asarray(order, np.int64)
        if self.selector == "topk":           # the top: the first batch_size regions of the population in rank order, this rank's own kept
            top = order[valid[order]][: batch]
            top = top[(top >= sub_s) & (top < sub_s + self.S)]
            loc = top - sub_s
            rec.rooms, rec.spin = room[top], spin[top]
            rec.picks, rec.pairs = np.arange(len(loc), dtype=np.int32), _Pairs(self.sp_cloud_h[loc], loc)
            return rec
        cand, ccloud, _, ntop = self._candidates(order, valid, cloud, batch)
        mine = (cand >= sub_s) & (cand < sub_s + self.S)
        gcand = cand[mine]
        cand, ccloud = gcand - sub_s, ccloud[mine] - sub_c
        ntop = np.concatenate([ntop, np.zeros(max(sub_c + self.B - len(ntop), 0), np.int64)])[sub_c: sub_c + self.B]
        rec.pairs = _Pairs(ccloud, cand)
        rec.rooms, rec.spin = room[gcand], spin[gcand]
        live = np.flatnonzero(ntop > 0)       # the clouds with picks are the clouds with candidates (a cloud offers min(2 x its picks, its regions))
        picks = int(ntop.sum())
        if picks == 0:
            rec.picks = np.zeros(0, np.int32)
            return rec
        n_c = np.bincount(ccloud, minlength=self.B)[live].astype(np.int64)
        if int(n_c.max()) > 8192:
            raise RuntimeError("edcd: a cloud has %d candidates; the batched farthest_superpoint_sample takes at most 8192" % int(n_c.max()))
        coff = np.concatenate([[0], np.cumsum(n_c)]).astype(np.int32)
        boff = np.concatenate([[0], np.cumsum(n_c * n_c)]).astype(np.int64)
        d_sel = DevArray.from_host(cand.astype(np.int32), st); d_coff = DevArray.from_host(coff, st); d_boff = DevArray.from_host(boff, st)
        d_ntop = DevArray.from_host(ntop[live].astype(np.int32), st)
        ntot, nmax, nsq = int(coff[-1]), int(n_c.max()), int(boff[-1])
        d_cen = DevArray((ntot, 3), np.float64); d_dir = DevArray((nsq,), np.float64); d_adj = DevArray((nsq,), np.float64)
        _lib.check(L.ssdr_select_set_chamfer_mode(0))        # the float64 chamfer, whatever chamfer_mode says (the device chain passes it itself)
        _lib.check(L.ssdr_cloud_graph_batch_dev(self.xyz.ptr, self.sp_off.ptr, self.sp_pts.ptr, d_sel.ptr, d_coff.ptr, d_boff.ptr, len(live), ntot, nmax, 0,
                                                d_cen.ptr, d_dir.ptr, d_adj.ptr, st))
        _lib.check(L.ssdr_select_set_chamfer_mode(self.chamfer_mode))
        rec.picks = d_out = DevArray((picks,), np.int32)
        _lib.check(L.ssdr_edcd_fps_batch_dev(d_cen.ptr, d_dir.ptr, d_coff.ptr, d_boff.ptr, d_ntop.ptr, len(live), nmax, picks, d_out.ptr, None, st))
        rec.keep += [d_sel, d_coff, d_boff, d_ntop, d_cen, d_dir, d_adj]
        return rec

    @property
    def comb_all(self):
        """the gathered candidate features of the last collected sharded selection (tests)"""
        _lib.sync()
        return self._collected.comb.to_host()[: self._collected.comb_n]

    def _select_collect(self):
        """wait for the FPS chain of _select_issue and read the selection back"""
        rec, self._pending = self._pending, None
        # Waits for the selection stream alone.  From ~20 tiles per GPU on the chain's FPS / k-center is a cooperative (multi-workgroup) launch: one that
        # was not co-resident reports it here, before its result is looked at, instead of returning a wrong selection
        _lib.check(_lib.lib().ssdr_select_status(self.sel_stream, None))
        sel, unl, where = {"device": self._collect_device, "sharded": self._collect_sharded, "topk": self._collect_topk, "host": self._collect_host}[rec.route](rec)
        # the device-flavour KNN calls cannot report what their kernels found (overflowed kd queue / node table / level limit, hand-over
        # list): ask once per batch, here where the host waits anyway — without waiting for the pyramids of the LATER batches that the
        # KNN stream already holds (the finished calls' tickets are looked at; Pipelined.finish / the sequential step wait for all)
        knn.knn_status(self.knn_stream if self.knn_stream is not None else self.stream, wait=not self.pipelined)
        if not self.pipelined:                               # sequential use: the front end of this batch has finished, ask it too
            _lib.check(_lib.lib().ssdr_grid_subsample_status(self.front_stream if self.front_stream is not None else self.stream, None))
        if len(sel) and int(np.min(sel)) < 0:                # (an aborted chain leaves -1 picks: never index the candidate list with them)
            raise RuntimeError("selection: the FPS / k-center chain left unset picks (an aborted cooperative launch)")
        if rec.emu_mod:                                      # (SSDR_EMULATE_WORLD: the picks index the repeated rows)
            sel = sel % rec.emu_mod
        si = np.asarray(sel, np.int64)
        if rec.comm is not None:
            where = self._sharded_where(where, si, rec)
        elif where.layout == _Picks.HOST:                    # decided on the host: the picks as region ids (label_selected uploads them)
            where.items = np.asarray(unl.b, np.int64)[si]
        self._collected, self._last_sel = rec, where
        self._selected = _Pairs(np.asarray(rec.rooms)[si], np.asarray(rec.spin)[si])      # (room id, superpoint in room)
        return sel, unl

    def _collect_device(self, rec):
        """a one-call chain's d_result: counts, picks and the candidate list in one read-back"""
        res = rec.buf.to_host(self.sel_stream)
        if self.selector == "coregcn":
            self.gcn_info = info = self.gcn_rows(info_only=True)
            sampler.gcn_status_check(info, self.room_ids)
        status = int(res[RES_STATUS])
        if status & ~3:
            raise RuntimeError("edcd_sampling: %s (status %d): nothing was selected" % (
                "a cloud has more than 8192 candidates" if status & 4 else "the picks do not fit the capacities", status))
        if status:
            raise RuntimeError("gcn_fps_sampling: the candidate rule produced more rows than the capacities allow (status %d)" % status)
        first = RES_HEADER + rec.max_select
        cand = res[first: first + int(res[RES_N_UNL])].astype(np.int64)
        rec.pairs = _Pairs(self.sp_cloud_h[cand], cand)      # (20 000 candidates in one AL round: the tuples are built when somebody reads them)
        rec.rooms, rec.spin = self._room_sp(cand)
        return res[RES_HEADER: RES_HEADER + int(res[RES_N_PICKS])].copy(), rec.pairs, _Picks(_Picks.RESULT0, rec.buf, rec.max_select)

    def _collect_topk(self, rec):
        """the top regions of the ranking (this rank's own): sel = arange"""
        res = rec.buf.to_host(self.sel_stream)
        loc = res[RES_HEADER: RES_HEADER + int(res[RES_N_UNL])].astype(np.int64)
        rec.pairs = _Pairs(self.sp_cloud_h[loc], loc)
        rec.rooms, rec.spin = self._room_sp(loc)
        return np.arange(len(loc), dtype=np.int32), rec.pairs, _Picks(_Picks.RESULT1, rec.buf, rec.max_select)

    def _collect_sharded(self, rec):
        """the sharded device-side rule: the plan (counts, global candidate list) and the replicated picks"""
        D = self.global_order; V = D["dev"]; rank = rec.comm.rank
        plan = rec.buf.to_host(self.sel_stream)
        sel = rec.picks.to_host(self.sel_stream)
        if plan[RES_STATUS] or plan[PLAN_OVERFLOW]:
            raise RuntimeError("gcn_fps_sharded: the candidate rule produced more rows than the capacities allow (status %d, %d)" % (
                int(plan[RES_STATUS]), int(plan[PLAN_OVERFLOW])))
        n_g, first = int(plan[PLAN_N_ALL]), _plan_gcand(rec.comm.world, V["nu_max"])
        rec.gcand = gcand = plan[first: first + n_g].astype(np.int64)
        loc = gcand[gcand // D["Smax"] == rank] - rank * D["Smax"]
        rec.pairs = _Pairs(self.sp_cloud_h[loc], loc)
        rec.rooms, rec.spin = D["room"][gcand], D["spin"][gcand]
        rec.comb, rec.comb_n = V["d_glob"], n_g + (V["n_lab_all"] if self.selector == "kcenter" else 0)
        if V["rep"] > 1:
            rec.emu_mod = n_g
        return sel, rec.pairs, _Picks(_Picks.REPLICATED, gcand=gcand)

    def _collect_host(self, rec):
        """decided on the host: the picks are a host array (the top of the host rule, a round without picks) or the chain's device array"""
        sel = rec.picks if isinstance(rec.picks, np.ndarray) else rec.picks.to_host(self.sel_stream)
        return sel, rec.pairs, _Picks(_Picks.HOST)

    def _sharded_where(self, where, si, rec):
        """Where a sharded selection's picks lie, for label_selected(comm=).  fps / k-center: the picks and the global candidate list are replicated; a rank's
        items are the picks whose region it holds (`own`: their positions among all picks, which is also their place in self.selected).  edcd / topk: a
        rank holds its own picks only.  Host rule: the items and their 64-bit walk keys (cloud key << 32 | position in pick order) are made here."""
        D = self.global_order if self.global_order is not None else self._dist
        Smax, rank, world = D["Smax"], rec.comm.rank, rec.comm.world
        if int(os.environ.get("SSDR_EMULATE_WORLD", "0")) > 1:
            return _Picks(_Picks.HOST, refuse="the selection ran under SSDR_EMULATE_WORLD (repeated rows: only its timing means anything)")
        if where.layout == _Picks.REPLICATED:                               # device rule, fps / k-center
            where.own = np.flatnonzero(where.gcand[si] // Smax == rank)
        elif where.layout != _Picks.HOST:                                   # device rule, edcd / topk: the chain's own result buffer
            where.own = np.arange(len(si))
        elif self.selector in ("fps", "kcenter"):                           # host rule: the picks index the global candidate list
            gid = np.asarray(rec.gcand, np.int64)[si]
            gc = D["gcloud"][gid]
            first = np.full(world * D["Bmax"], 1 << 30, np.int64)
            np.minimum.at(first, gc, np.arange(len(gid)))                  # a cloud's first appearance among ALL picks
            where.own = own = np.flatnonzero(gid // Smax == rank)
            where.items, where.keys = gid[own] - rank * Smax, (first[gc[own]] << 32) | own
        else:                                                               # host rule, edcd / topk
            ids = np.asarray(rec.pairs.b, np.int64)[si]
            r = np.flatnonzero(D["valid"][rec.gorder])                      # a cloud's first place in the global ranking among the regions that compete
            key = np.full(world * D["Bmax"], 0x7f7f7f7f, np.int64)
            np.minimum.at(key, D["gcloud"][rec.gorder[r]], r)
            where.items, where.keys, where.own = ids, (key[D["gcloud"][rank * Smax + ids]] << 32) | np.arange(len(ids)), np.arange(len(ids))
        return where

    def gcn_rows(self, info_only=False):
        """what the last "coregcn" selection left on the device: (evaluation rows [rows,129] float64, trained parameters, (loss at step 0, loss after the
        last step), info) — info = [status bits, first single-row cloud, substituted values, form]"""
        L, st = _lib.lib(), self.sel_stream
        p_rows, cap, p_par, p_loss, p_info = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(L.ssdr_gcn_sampling_rows(st, C.byref(p_rows), C.byref(cap), C.byref(p_par), C.byref(p_loss), C.byref(p_info)))
        info = np.empty(8, np.int32)
        _lib.check(L.ssdr_memcpy_d2h_on(_lib.ptr(info), p_info.value, info.nbytes, st))
        if info_only:
            return info
        rows = np.empty((int(cap.value), 129), np.float64); par = np.empty(4353, np.float32); loss = np.empty(2, np.float32)
        _lib.check(L.ssdr_memcpy_d2h_on(_lib.ptr(rows), p_rows.value, rows.nbytes, st)); _lib.check(L.ssdr_memcpy_d2h_on(_lib.ptr(par), p_par.value, par.nbytes, st))
        _lib.check(L.ssdr_memcpy_d2h_on(_lib.ptr(loss), p_loss.value, loss.nbytes, st))
        return rows, par, loss, info

    @property
    def selected(self):
        """the picks as [(room id, superpoint in room), ...] — a plain list, built on first access"""
        v = self.__dict__.get("_selected")
        return v.tolist() if isinstance(v, _Pairs) else v

    @selected.setter
    def selected(self, value):
        self._selected = value

    # ---- the oracle: pseudo labels for the picks of the last selection (sampler2.py:124-216) ------------------
    def set_pseudo_gt(self, pseudo_gt):
        """the resident pseudo labels' content: [2, n] over all points (row 0 labelled flag, row 1 label), or one [2, n_c] array per cloud"""
        a = np.concatenate([np.asarray(p, np.float32) for p in pseudo_gt], axis=1) if isinstance(pseudo_gt, (list, tuple)) else np.asarray(pseudo_gt, np.float32)
        assert a.shape == (2, self.n_pts), "pseudo_gt must be [2, %d]" % self.n_pts
        self.pseudo_mask, self.pseudo_label = DevArray.from_host(np.ascontiguousarray(a[0])), DevArray.from_host(np.ascontiguousarray(a[1]))
        return self

    def label_selected(self, mode="NAIL", threshold=0.9, min_size=None, budget=None, comm=None):
        """_help() / oracle_labeling() for every cloud that received picks (sampler2.py:124-216, called from sampling() :676-684, :775-781, :796-806), on
        the device and from the device buffers of the last selection: the picks become pseudo labels while the click budget (default: the round's
        batch_size, as sampling() sets it) lasts.  Afterwards self.labeled, the skip mask and selected_class_list are what set_labeled() would
        produce for the next round: step_selection() can be called again.  Returns a LabelResult.
        comm: the communicator of the last selection (a sharded round): every rank judges its own picks, the verdict records are all-gathered on the
        selection stream, every rank runs the same walk over all of them and applies its own.  The counters, budget_left and the class list are then
        global and equal on all ranks; `used` / `walk_pos` are this rank's used picks and their positions in the global walk."""
        if self.selector in REGION_SAMPLERS:
            return self._region_label(mode, threshold, min_size, budget, comm)
        last = None if self._collected is None else self._collected.comm
        if last is not None and comm is None:
            raise ValueError("label_selected: the last selection ran with a communicator; the budget walk is global over all ranks' picks: pass that "
                             "communicator (label_selected(comm=comm))")
        if comm is not None:
            if comm is not last:
                raise ValueError("label_selected: comm must be the communicator of the last selection")
            return self._label_selected_sharded(comm, mode, threshold, min_size, budget)
        where, m, budget, min_size = self._label_begin(None, mode, budget, min_size)
        L, st, T = _lib.lib(), self.sel_stream, self._sel_static
        edcd = self.selector == "edcd"
        d_key = DevArray((max(self.B, 1),), np.int32) if edcd else None
        if where.layout == _Picks.HOST:
            items = where.items
            M = len(items)
            d_items = DevArray.from_host(np.concatenate([items, [0]]).astype(np.int32), st); d_n = DevArray.from_host(np.array([M], np.int32), st)
            if edcd:
                _lib.check(L.ssdr_oracle_label_items_dev(None, 0, 0, self.sorted_inds.ptr, self.S, T["d_lab"].ptr, self.d_sp_cloud.ptr, self.B, None, 0, None, d_key.ptr, st))
        else:
            M = where.max_select
            d_items = DevArray((max(M, 1),), np.int32); d_n = DevArray((1,), np.int32)
            _lib.check(L.ssdr_oracle_label_items_dev(where.buf.ptr, where.layout, M, self.sorted_inds.ptr if edcd else None, self.S, T["d_lab"].ptr,
                                                     self.d_sp_cloud.ptr, self.B, d_items.ptr, M, d_n.ptr, d_key.ptr if edcd else None, st))
        nc = int(self.cfg.num_classes)
        cap = max(1, min(M * nc, max(budget, 0) + nc + 1))
        d_budget = DevArray.from_host(np.array([budget], np.int64), st)
        d_used, d_proc = DevArray((max(M, 1),), np.uint8), DevArray((max(M, 1),), np.int32)
        d_labeled = DevArray.from_host(self.labeled_mask.astype(np.uint8) if self.S else np.zeros(1, np.uint8), st)
        d_cls, d_out = DevArray((cap,), np.int32), DevArray((12,), np.int64)
        _lib.check(L.ssdr_oracle_label_dev(self.tile_l.ptr, self.cls.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, self.d_sp_cloud.ptr, self.B,
                                           d_items.ptr, d_n.ptr, M, d_key.ptr if edcd else None, int(self.sp_size_h.max()) if self.S else 1, max(nc, 1), nc, m,
                                           float(threshold), min_size, d_budget.ptr, self.pseudo_mask.ptr, self.pseudo_label.ptr, d_used.ptr, d_labeled.ptr,
                                           d_cls.ptr, cap, d_proc.ptr, d_out.ptr, st))
        out = d_out.to_host(st)                              # waits for the selection stream alone
        sampler.label_status_check(int(out[8]))
        used_f, proc = d_used.to_host(st), d_proc.to_host(st)
        n_items = int(d_n.to_host(st)[0])
        proc = proc[:n_items]
        upos = proc[used_f[proc] != 0]                       # the used picks in the order the walk met them
        return self._label_end(out, d_cls, d_labeled, upos, np.flatnonzero(used_f[proc] != 0))

    def _label_begin(self, comm, mode, budget, min_size):
        """what both forms of label_selected start with: the picks' location, the mode, the click budget (default: the round's batch_size, one number for
        all ranks of a sharded round), min_size, and pseudo labels to write into"""
        where = self._last_sel
        if where is None:
            raise RuntimeError("label_selected: no selection to label (run step_selection(%s) / step(%s) first)" % (("", "") if comm is None else ("comm", "comm")))
        if where.refuse:
            raise ValueError("label_selected: " + where.refuse)
        m = sampler.label_mode([mode] if isinstance(mode, str) else mode)
        batch = int(self._sel_static["batch"] if comm is None else self._dist_setup(comm)["batch"])
        if self.pseudo_mask is None:
            self.set_pseudo_gt(np.zeros((2, self.n_pts), np.float32))
        return where, m, batch if budget is None else int(budget), self.min_size if min_size is None else int(min_size)

    def _label_end(self, out, d_cls, d_labeled, used_at, walk_pos):
        """what both forms end with: the new entries of the class list (global, identical on every rank of a sharded round), the labelled set from the
        device mask (set_labeled drops _dist: a sharded next round redoes the global draw), the picks spent, the LabelResult; used_at: the used picks'
        places in self.selected, in the order the walk met them"""
        st = self.sel_stream
        sel_pairs = self.__dict__.get("_selected")
        used = _Pairs(np.asarray(sel_pairs.a)[used_at], np.asarray(sel_pairs.b)[used_at])
        entries = d_cls.to_host(st)[: int(out[6])]
        self._class_list_h = np.concatenate([self._class_list_h, entries]).astype(np.int32)
        self.selected_class_list = DevArray.from_host(self._class_list_h)
        mask = d_labeled.to_host(st)[: self.S] != 0
        self.set_labeled({b: set(np.flatnonzero(mask & (self.sp_cloud_h == b)).tolist()) for b in range(self.B)})
        self._last_sel = None                                # (these picks are spent)
        return LabelResult(self, dict(zip(sampler.LABEL_COUNTERS, (int(x) for x in out[:6]))), int(out[7]), used, entries,
                           dict(wave=int(out[10]), block=int(out[11])), walk_pos)

    def _label_selected_sharded(self, comm, mode, threshold, min_size, budget):
        """label_selected over a sharded round: walk keys -> verdict half -> all-gather of the records (the fourth exchange) -> walk half"""
        where, m, budget, min_size = self._label_begin(comm, mode, budget, min_size)
        L, st = _lib.lib(), self.sel_stream
        D = self._dist_setup(comm); V = D["dev"]
        W, rank, Smax, Bmax, batch = comm.world, comm.rank, D["Smax"], D["Bmax"], int(D["batch"])
        # the record slots per rank: the most picks any rank can hold, from what _dist_setup exchanged
        # (fps / kcenter: the replicated chain may hand ALL picks to one rank, and the all-gather needs the same slot count on every rank)
        M = {"edcd": min(batch, int(D["nvalid_all"].max())), "topk": min(batch, Smax)}.get(self.selector, V["picks"])
        M = max(int(M), 1)
        d_items, d_n, d_keys = DevArray((M,), np.int32), DevArray((1,), np.int32), DevArray((M,), np.uint64)
        if where.layout == _Picks.HOST:                       # host rule: items and keys were made on the host
            k = len(where.items)
            assert k <= M
            _lib.check(L.ssdr_memcpy_h2d_on(d_items.ptr, _lib.ptr(np.ascontiguousarray(where.items, np.int32)), 4 * k, st))
            _lib.check(L.ssdr_memcpy_h2d_on(d_keys.ptr, _lib.ptr(np.ascontiguousarray(where.keys).astype(np.uint64)), 8 * k, st))
            _lib.check(L.ssdr_memcpy_h2d_on(d_n.ptr, _lib.ptr(np.array([k], np.int32)), 4, st))
        elif where.layout == _Picks.REPLICATED:               # the replicated picks over the replicated global candidate list
            _lib.check(L.ssdr_oracle_label_keys_dev(V["d_out"].ptr, V["picks"], V["d_plan"].ptr + 4 * PLAN_N_ALL, V["d_plan"].ptr + 4 * _plan_gcand(W, V["nu_max"]),
                                                    W * V["nu_max"], D["d_gcloud"].ptr, Smax, W * Bmax, rank, W, None, d_items.ptr, d_n.ptr, M, d_keys.ptr, st))
        else:                                                 # the rank's own picks; a cloud's key is its first place in the global ranking
            d_key = DevArray((W * Bmax,), np.int32)
            ms = min(where.max_select, M)
            _lib.check(L.ssdr_oracle_label_items_dev(where.buf.ptr, where.layout, where.max_select, D["d_ord"].ptr, W * Smax, V["d_glab"].ptr, D["d_gcloud"].ptr,
                                                     W * Bmax, d_items.ptr, ms, d_n.ptr, d_key.ptr, st))
            _lib.check(L.ssdr_oracle_label_keys_dev(None, 0, None, None, 0, D["d_gcloud"].ptr, Smax, W * Bmax, rank, W, d_key.ptr, d_items.ptr, d_n.ptr, M, d_keys.ptr, st))
        nc = int(self.cfg.num_classes)
        max_region = int(self.sp_size_h.max()) if self.S else 1
        d_send, d_gath = DevArray((M * _lib.LABEL_RECORD_BYTES,), np.uint8), DevArray((W, M * _lib.LABEL_RECORD_BYTES), np.uint8)
        _lib.check(L.ssdr_oracle_label_verdict_dev(self.tile_l.ptr, self.cls.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, d_items.ptr, d_n.ptr, M, d_keys.ptr,
                                                   max_region, max(nc, 1), nc, m, float(threshold), min_size, d_send.ptr, st))
        comm.allgather_(d_send, d_gath, st)                  # exchange 4: every rank's verdict records
        cap = max(1, min(W * M * nc, max(budget, 0) + nc + 1))
        d_budget = DevArray.from_host(np.array([budget], np.int64), st)
        d_used, d_pos = DevArray((M,), np.uint8), DevArray((M,), np.int32)
        d_labeled = DevArray.from_host(self.labeled_mask.astype(np.uint8) if self.S else np.zeros(1, np.uint8), st)
        d_cls, d_out = DevArray((cap,), np.int32), DevArray((12,), np.int64)
        _lib.check(L.ssdr_oracle_label_walk_dev(d_gath.ptr, rank, W, self.cls.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, d_items.ptr, d_n.ptr, M, max_region,
                                                nc, d_budget.ptr, self.pseudo_mask.ptr, self.pseudo_label.ptr, d_used.ptr, d_labeled.ptr, d_cls.ptr, cap, d_pos.ptr,
                                                d_out.ptr, st))
        out = d_out.to_host(st)                              # waits for the selection stream alone
        sampler.label_status_check(int(out[8]))
        n_items = int(d_n.to_host(st)[0])
        used_f, pos = d_used.to_host(st)[:n_items], d_pos.to_host(st)[:n_items]
        own = np.asarray(where.own, np.int64)
        if len(own) != n_items:
            raise RuntimeError("label_selected: the device found %d picks of this rank, the selection read back %d" % (n_items, len(own)))
        slots = np.flatnonzero(used_f != 0)
        slots = slots[np.argsort(pos[slots], kind="stable")]      # this rank's used picks in the order the global walk met them
        return self._label_end(out, d_cls, d_labeled, own[slots], pos[slots].astype(np.int64))

    # ---- the seed, random and label-all rounds (sampler2.py:344-520): no scoring, no network outputs ----------------
    def _region_dist(self, comm):
        """The tables of ONE sharded seed / random / label-all round, exchanged when it begins (nothing is kept between rounds: rooms, regions and labels may
        all have changed): every rank's region, cloud and unlabelled count.  The ranks hold contiguous shares of the clouds in rank order, so the union has a
        global region id (the regions of the ranks before + the local id) and every rank's count table takes the largest cloud count of any rank."""
        sb = comm.allgather_host(np.array([self.S, self.B, int((~self.labeled_mask).sum())], np.int64))
        S_all, CS = sb[:, 0], max(int(sb[:, 1].max()), 1)
        return dict(S_all=S_all, first=int(S_all[: comm.rank].sum()), S_total=int(S_all.sum()), Smax=max(int(S_all.max()), 1), CS=CS, B_total=int(sb[:, 1].sum()),
                    unl=int(sb[:, 2].sum()), d_u=DevArray((CS + 1,), np.int32), d_u_all=DevArray((comm.world, CS + 1), np.int32))

    def _unl_host(self):
        """draws="host": every cloud's unlabelled list (ids inside the cloud) as total_obj["unlabeled"] holds it; ascending when first made"""
        if self._unl_lists is None:
            base = np.concatenate([np.asarray(self.sp_base, np.int64), [self.S]])
            lists = {}
            for b in range(self.B):
                ids = np.flatnonzero(~self.labeled_mask[base[b]:base[b + 1]]).tolist()
                if ids:
                    lists[b] = ids
            self._unl_lists = lists
        return self._unl_lists

    @property
    def unlabeled_lists(self):
        """total_obj["unlabeled"] as the seed / random / label-all rounds keep it: {cloud: [region id inside the cloud, ...]}, live clouds only; with
        draws="host" in the reference's own order, otherwise ascending"""
        return self._unl_host()

    def _region_begin(self, comm=None):
        """the device state one seed / random / label-all round keeps across its iterations.  comm: a sharded round — R["unl"] is then the unlabelled
        regions of ALL ranks, kept from replicated device words alone: every rank takes the loop's decisions from it, never from its own mask"""
        st = self.sel_stream
        _region_check_comm(self.selector, comm, self.draws)
        D = None if comm is None else self._region_dist(comm)
        if self.S == 0 or (D is not None and (D["S_all"] == 0).any()):      # (the exchanged counts: raised on every rank)
            raise ValueError("the seed / random / label-all samplers need at least one region" + ("" if comm is None else " on every rank"))
        if D is not None and D["S_total"] > 0x3fffffff:                     # (a low rank's own first_region + S does not show it)
            raise ValueError("the sharded seed / random / label-all samplers take at most 0x3fffffff regions over all ranks (%d)" % D["S_total"])
        if self.pseudo_mask is None:
            self.set_pseudo_gt(np.zeros((2, self.n_pts), np.float32))
        R = dict(d_labeled=DevArray.from_host(self.labeled_mask.astype(np.uint8), st), d_items=DevArray((self.S if D is None else D["Smax"],), np.int32),
                 d_n=DevArray((1,), np.int32), d_info=DevArray((8,), np.int64), d_budget=DevArray((1,), np.int64), labeled=self.labeled_mask.copy(), it=0, drawn=[],
                 infos=[], picks=None, items=None, comm=comm, positions=[], D=D)
        if comm is not None:
            R["d_pos"], R["unl"] = DevArray((D["Smax"],), np.int32), D["unl"]
        return R

    @staticmethod
    def _region_all_labeled(R):
        return R["labeled"].all() if R["comm"] is None else R["unl"] <= 0

    def _region_draw(self, R, click, mode, round_num):
        """One iteration's item list into R["d_items"] / R["d_n"]: `click` elements of range(total_num) shared among the live clouds, every cloud's picks
        (mode REGION_RANDOM), or every unlabelled region (REGION_ALL).  *R["d_budget"] holds `click`.  -> (items as global region ids, info)"""
        L, st, comm = _lib.lib(), self.sel_stream, R["comm"]
        T = self.total_num if self.total_num is not None else self.S if comm is None else R["D"]["S_total"]
        if mode == sampler.REGION_RANDOM and click > T:
            raise ValueError("Cannot take a larger sample than population when 'replace=False' (%d clicks of total_num = %d)" % (click, T))
        if comm is not None:
            # the draw in two halves around one all-gather of the ranks' count tables, all on the selection stream; every word the host decides on below is
            # replicated.  items: this rank's, as local ids; info["pos"]: their places in the union's list
            D = R["D"]
            _lib.check(L.ssdr_region_draw_count_dev(R["d_labeled"].ptr, self.d_sp_cloud.ptr, self.S, max(self.B, 1), D["d_u"].ptr, D["CS"], st))
            comm.allgather_(D["d_u"], D["d_u_all"], st)
            _lib.check(L.ssdr_region_draw_sharded_dev(self.draw_seed & 0xffffffffffffffff, int(round_num) & 0xffffffff, R["it"], mode, self.draw_key_bits, D["first"], comm.rank,
                                                      comm.world, D["d_u_all"].ptr, D["CS"], R["d_labeled"].ptr, self.d_sp_cloud.ptr, self.S, max(self.B, 1), T, R["d_budget"].ptr,
                                                      R["d_items"].ptr, R["d_pos"].ptr, self.S, R["d_n"].ptr, R["d_info"].ptr, st))
            w = R["d_info"].to_host(st)                           # waits for the selection stream alone
            # (bit 2, the one word of d_info that is this rank's own, cannot be set: the item list holds S items; the raises below are from replicated bits)
            sampler.region_draw_status_check(int(w[5]) & ~sampler.DRAW_ST_ITEMS, int(w[1]), T)
            own = int(w[6])
            items = R["d_items"].to_host(st)[:own].astype(np.int64)
            info = dict(live=int(w[0]), k=int(w[1]), items=int(w[2]), remain=int(w[3]), each=None, own=own, pos=R["d_pos"].to_host(st)[:own].astype(np.int64),
                        unlabeled=int(w[2] + w[4]))
            if self.record_shares:
                info["each"] = np.zeros(info["live"], np.int32)
                _lib.check(L.ssdr_region_draw_shares(st, _lib.ptr(info["each"]), info["live"]))
            R["positions"].append(info["pos"])
        elif self.draws == "host":
            unl = self._unl_host()
            if mode == sampler.REGION_ALL:
                picks, each, remain = [(c, list(unl[c])) for c in unl], np.array([len(unl[c]) for c in unl], np.int32), 0
            else:
                picks, each, remain = sampler.seed_iteration_host(T, unl, click, self.draw_rng)
            items = np.array([self.sp_base[c] + s for c, sps in picks for s in sps], np.int64)
            if len(items):
                _lib.check(L.ssdr_memcpy_h2d_on(R["d_items"].ptr, _lib.ptr(np.ascontiguousarray(items, np.int32)), 4 * len(items), st))
            _lib.check(L.ssdr_memcpy_h2d_on(R["d_n"].ptr, _lib.ptr(np.array([len(items)], np.int32)), 4, st))
            info = dict(live=len(each), k=int(click), items=len(items), remain=int(remain), each=np.asarray(each, np.int64))
            R["picks"] = picks
        else:
            _lib.check(L.ssdr_region_draw_dev(self.draw_seed & 0xffffffffffffffff, int(round_num) & 0xffffffff, R["it"], mode, self.draw_key_bits, 0, R["d_labeled"].ptr,
                                              self.d_sp_cloud.ptr, self.S, max(self.B, 1), T, R["d_budget"].ptr, R["d_items"].ptr, self.S, R["d_n"].ptr, R["d_info"].ptr, st))
            w = R["d_info"].to_host(st)                           # waits for the selection stream alone
            sampler.region_draw_status_check(int(w[5]), int(w[1]), T)
            items = R["d_items"].to_host(st)[: int(w[2])].astype(np.int64)
            info = dict(live=int(w[0]), k=int(w[1]), items=int(w[2]), remain=int(w[3]), each=None)
            if self.record_shares:
                info["each"] = np.zeros(info["live"], np.int32)
                _lib.check(L.ssdr_region_draw_shares(st, _lib.ptr(info["each"]), info["live"]))
        R["items"], R["info"] = items, info
        R["drawn"].append(items); R["infos"].append(info)
        return items, info

    def _region_set_budget(self, R, click):
        _lib.check(_lib.lib().ssdr_memcpy_h2d_on(R["d_budget"].ptr, _lib.ptr(np.array([int(click)], np.int64)), 8, self.sel_stream))

    def _region_select(self, comm=None):
        """step_selection() of "random" / "all": iteration 0's picks for the round's batch_size clicks — (arange, the picks as (cloud, region))"""
        R = self._region_begin(comm)
        # (a sharded round: sampling()'s batch_size is ONE number for all ranks, as _dist_setup has it)
        R["click0"] = int(self._sel_static["batch"] if comm is None or self.batch_size is not None else self.select_per_tile * R["D"]["B_total"])
        self._region_set_budget(R, R["click0"])
        items, _ = self._region_draw(R, R["click0"], sampler.REGION_ALL if self.selector == "all" else sampler.REGION_RANDOM, self.round_num)
        self._drawn0, self._last_sel = R, None
        self._selected = _Pairs(*self._room_sp(items))
        return np.arange(len(items), dtype=np.int32), _Pairs(self.sp_cloud_h[items], items)

    def _region_label(self, mode, threshold, min_size, budget, comm):
        """label_selected() of "random" / "all": the walk over iteration 0's items, then (random) further draws and walks while clicks and unlabelled
        regions last — RandomSampler._iteration's recursion (sampler2.py:463-493) as a loop that max_iter ends.
        comm: the communicator iteration 0 was drawn with.  One iteration's walk is then the sharded form (the items' places in the union's list as walk
        keys -> verdict half -> all-gather of the records -> walk half on the iteration's d_labeled), and the loop is steered by the walk's replicated
        d_out and the draw's replicated d_info alone: all ranks draw again, stop and raise together."""
        _region_check_comm(self.selector, comm, self.draws)
        R = self._drawn0
        if R is None:
            raise RuntimeError("label_selected: no selection to label (run step_selection() first)")
        if R["comm"] is not comm:
            raise ValueError("label_selected: comm must be the communicator of the last selection (iteration 0 was drawn %s one)" % ("without" if R["comm"] is None else "with"))
        m = sampler.label_mode([mode] if isinstance(mode, str) else mode)
        if m == 1 and not self._pred_resident:
            raise ValueError('label_selected: mode="NAIL" with selector="%s" needs predicted classes resident from an earlier prediction pass (the reference '
                             'passes prob_class=None and fails on the first impure region); "dominant" always works' % self.selector)
        rand = self.selector == "random"
        if budget is not None and int(budget) != R["click0"]:
            if rand:
                raise ValueError("label_selected: iteration 0 was drawn for batch_size = %d clicks; a round of %d clicks needs HotPath(batch_size=%d)" % (R["click0"], int(budget), int(budget)))
            R["click0"] = int(budget)                             # (label-all draws nothing: any budget walks the same list)
            self._region_set_budget(R, R["click0"])
        min_size = (self.min_size if min_size is None else int(min_size)) if rand else 1      # AllSampler passes min_size=1 (sampler2.py:449)
        click, status = R["click0"], 0
        counters, entries, used_ids, forms, walk_pos = np.zeros(6, np.int64), [], [], np.zeros(2, np.int64), []
        walk = self._region_walk if comm is None else self._region_walk_sharded
        while True:
            out, ent, used, wpos = walk(R, click, m, float(threshold), min_size)
            self._region_spent(R, used)
            counters += out[:6]; forms += out[10:12]; entries.append(ent); used_ids.append(used); walk_pos.append(wpos)
            click = int(out[7])
            R["it"] += 1
            if not rand or click <= 0 or self._region_all_labeled(R):
                break
            if R["it"] >= self.max_iter:                         # only regions below min_size are left: the reference recurses for ever
                status |= sampler.ST_MAX_ITER
                break
            self._region_draw(R, click, sampler.REGION_RANDOM, self.round_num)
        return self._region_end(R, counters, click, np.concatenate(used_ids), np.concatenate(entries), dict(wave=int(forms[0]), block=int(forms[1])), status,
                                walk_pos if comm is not None else None)

    def _region_walk(self, R, click, m, threshold, min_size):
        """the budget walk over one iteration's items -> (d_out, the new class entries, the used items in walk order, None)"""
        L, st, nc = _lib.lib(), self.sel_stream, int(self.cfg.num_classes)
        items, M = R["items"], len(R["items"])
        cap = max(1, min(M * nc, max(click, 0) + nc + 1))
        d_used, d_proc = DevArray((max(M, 1),), np.uint8), DevArray((max(M, 1),), np.int32)
        d_cls, d_out = DevArray((cap,), np.int32), DevArray((12,), np.int64)
        _lib.check(L.ssdr_oracle_label_dev(self.tile_l.ptr, self.cls.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, self.d_sp_cloud.ptr, max(self.B, 1),
                                           R["d_items"].ptr, R["d_n"].ptr, M, None, int(self.sp_size_h.max()), max(nc, 1), nc, m, threshold, min_size, R["d_budget"].ptr,
                                           self.pseudo_mask.ptr, self.pseudo_label.ptr, d_used.ptr, R["d_labeled"].ptr, d_cls.ptr, cap, d_proc.ptr, d_out.ptr, st))
        out = d_out.to_host(st)                                  # the budget and the counters: one read per iteration
        sampler.label_status_check(int(out[8]))
        used_f, proc = d_used.to_host(st)[:M], d_proc.to_host(st)[:M]
        return out, d_cls.to_host(st)[: int(out[6])], items[proc[used_f[proc] != 0]] if M else items, None

    def _region_walk_sharded(self, R, click, m, threshold, min_size):
        """the same walk over ALL ranks' items of one iteration: the items' places in the union's list as walk keys -> verdict half -> all-gather of the
        records -> walk half on the iteration's d_labeled.  d_out is global and equal on every rank; it also gives R["unl"], the regions left unlabelled over
        all ranks.  -> (d_out, the new class entries (global), this rank's used items in walk order, their walk positions)"""
        L, st, nc, comm = _lib.lib(), self.sel_stream, int(self.cfg.num_classes), R["comm"]
        D, W, items, n = R["D"], comm.world, R["items"], len(R["items"])
        # the record slots per rank, one number on every rank: no rank holds more items than clicks are drawn for, or than the largest share has regions
        M = max(1, D["Smax"] if self.selector == "all" else min(click, D["Smax"]))
        keys = np.zeros(M, np.uint64); keys[:n] = R["info"]["pos"]
        d_keys = DevArray.from_host(keys, st)
        max_region = int(self.sp_size_h.max())
        d_send, d_gath = DevArray((M * _lib.LABEL_RECORD_BYTES,), np.uint8), DevArray((W, M * _lib.LABEL_RECORD_BYTES), np.uint8)
        _lib.check(L.ssdr_oracle_label_verdict_dev(self.tile_l.ptr, self.cls.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, R["d_items"].ptr, R["d_n"].ptr, M,
                                                   d_keys.ptr, max_region, max(nc, 1), nc, m, threshold, min_size, d_send.ptr, st))
        comm.allgather_(d_send, d_gath, st)
        cap = max(1, min(W * M * nc, max(click, 0) + nc + 1))
        d_used, d_wpos = DevArray((M,), np.uint8), DevArray((M,), np.int32)
        d_cls, d_out = DevArray((cap,), np.int32), DevArray((12,), np.int64)
        _lib.check(L.ssdr_oracle_label_walk_dev(d_gath.ptr, comm.rank, W, self.cls.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, R["d_items"].ptr, R["d_n"].ptr, M,
                                                max_region, nc, R["d_budget"].ptr, self.pseudo_mask.ptr, self.pseudo_label.ptr, d_used.ptr, R["d_labeled"].ptr, d_cls.ptr, cap,
                                                d_wpos.ptr, d_out.ptr, st))
        out = d_out.to_host(st)
        sampler.label_status_check(int(out[8]))
        R["unl"] = R["info"]["unlabeled"] - int(out[9])          # (the draw's unlabelled regions less the items the walk used, both over all ranks)
        used_f, wpos = d_used.to_host(st)[:n], d_wpos.to_host(st)[:n]
        slots = np.flatnonzero(used_f != 0)
        slots = slots[np.argsort(wpos[slots], kind="stable")]
        return out, d_cls.to_host(st)[: int(out[6])], items[slots], wpos[slots].astype(np.int64)

    def _region_spent(self, R, used):
        """what _help / _help_seed do to the unlabelled lists once a walk has used `used` (global ids) of the iteration's items"""
        R["labeled"][used] = True
        if self.draws == "host":
            gone = set(int(x) for x in used)
            for c, sps in R["picks"]:
                sampler.remove_used(self._unl_lists, c, [s for s in sps if self.sp_base[c] + s in gone])

    def _region_end(self, R, counters, budget_left, used_ids, entries, forms, status, walk_pos=None):
        st = self.sel_stream
        self._class_list_h = np.concatenate([self._class_list_h, entries]).astype(np.int32)
        self.selected_class_list = DevArray.from_host(self._class_list_h)
        mask = R["d_labeled"].to_host(st)[: self.S] != 0
        lists = self._unl_lists
        ids = np.flatnonzero(mask)                               # (ascending, and so are the clouds: one cut per cloud)
        parts = np.split(ids, np.searchsorted(ids, np.asarray(self.sp_base[1:], np.int64)))
        self.set_labeled({b: set(parts[b].tolist()) for b in range(self.B)})
        self._unl_lists = lists if self.draws == "host" else None      # (set_labeled drops them: these ARE the lists behind the new mask)
        return LabelResult(self, dict(zip(sampler.LABEL_COUNTERS, (int(x) for x in counters))), int(budget_left), _Pairs(*self._room_sp(np.asarray(used_ids, np.int64))),
                           np.asarray(entries, np.int32), forms, walk_pos, iterations=R["it"], drawn=R["drawn"], status=status, draw_info=R["infos"],
                           item_pos=R["positions"] if R["comm"] is not None else None)

    def seed_round(self, number, round_num=0, comm=None):
        """SeedSampler.sampling (sampler2.py:344-408): `number` regions drawn among the clouds and labelled PRECISELY (every point its own ground truth,
        no budget, no min_size, no class entries); a cloud smaller than its share is taken whole and the shortfall is drawn again, until none is left.
        Returns a LabelResult: counters sp_num / p_num, budget_left = the remainder that could not be placed.
        comm: the clouds are sharded over the communicator's ranks; every rank labels its own items, the counters (summed on the selection stream), the
        remainder and the iterations are those of all ranks."""
        L, st = _lib.lib(), self.sel_stream
        R = self._region_begin(comm)
        remain, status = int(number), 0
        sp_num = p_num = 0
        max_region = int(self.sp_size_h.max()) if self.S else 1
        d_out = DevArray((3,), np.int64)
        while remain > 0 and not self._region_all_labeled(R):
            if R["it"] >= self.max_iter:
                status |= sampler.ST_MAX_ITER
                break
            self._region_set_budget(R, remain)
            items, info = self._region_draw(R, remain, sampler.REGION_RANDOM, round_num)
            _lib.check(L.ssdr_seed_label_dev(self.tile_l.ptr, self.n_pts, self.sp_off.ptr, self.sp_pts.ptr, self.S, R["d_items"].ptr, R["d_n"].ptr, len(items), max_region,
                                             self.pseudo_mask.ptr, self.pseudo_label.ptr, R["d_labeled"].ptr, d_out.ptr, st))
            if comm is not None:
                comm.allreduce_sum_(d_out, st)                   # (a status bit of any rank stays non-zero in the sum)
                R["unl"] = info["unlabeled"] - info["items"]
            out = d_out.to_host(st)
            sampler.label_status_check(int(out[2]) if comm is None else 4 * int(out[2] != 0))
            sp_num += int(out[0]); p_num += int(out[1])
            self._region_spent(R, items)
            remain = info["remain"]
            R["it"] += 1
        counters = np.array([sp_num, p_num, 0, 0, 0, 0], np.int64)
        used = np.concatenate(R["drawn"]) if R["drawn"] else np.zeros(0, np.int64)
        return self._region_end(R, counters, remain, used, np.zeros(0, np.int32), dict(wave=0, block=0), status)

    def step(self, comm=None, timed_stages=False):
        """One pass of the hot path over the loaded batch of rooms.  Returns the selected candidate indices."""
        t = [time.perf_counter()]

        def mark():
            if timed_stages:
                _lib.sync(); t.append(time.perf_counter())
        self._front_end(); mark()
        self._pyramid(); mark()
        self._infer(); mark()
        self._score_async(comm); mark()
        out = self._select(comm); mark()
        if timed_stages:
            self.timing = dict(zip(("subsample+tile", "knn_pyramid", "randla_infer", "score", "select"), np.diff(t) * 1e3))
        return out


def _region_check_comm(selector, comm, draws):
    """what the seed / random / label-all rounds ask of a communicator; raised before any exchange, so on every rank"""
    if comm is None:
        return
    if not all(hasattr(comm, a) for a in ("rank", "world", "allgather_", "allgather_host", "allreduce_sum_")):
        raise ValueError('selector="%s": comm = %r is not a communicator (ssdr_al.distributed.Comm)' % (selector, comm))
    if draws == "host":
        raise ValueError('draws="host" with a communicator: the RandomState chain is sequential over all clouds\' lists, which no rank holds; use draws="device"')


def _new_stream():
    st = C.c_void_p()
    _lib.check(_lib.lib().ssdr_stream_create(C.byref(st)))
    return st.value


class LabelResult:
    """What HotPath.label_selected / ALRound.label hand back: `mask` / `label` (device, float32 [n]: the two rows of pseudo_gt over all points, the
    HotPath's own resident arrays), `used` as (room id, superpoint in room) pairs in the order the walk met them, the six `counters` of the
    reference's `w`, `budget_left` (may be negative), `class_entries` appended to selected_class_list, `forms`: regions judged per kernel form,
    `walk_pos`: the position of every entry of `used` in the walk, `iterations` / `drawn` / `status`: the draw iterations of a seed, random or
    label-all round, their items and why the loop stopped (budget_left is the seed round's remainder).  After a sharded labelling the counters, budget_left, class_entries and forms are
    global (equal on all ranks), `used` / `walk_pos` this rank's share of the global walk.  After a sharded seed, random or label-all round `drawn` are this
    rank's items per iteration, `item_pos` their positions in the union's item list and `walk_pos` the used regions' walk positions per iteration (lists
    of arrays); `iterations`, `status` and `draw_info` (k, live clouds, items, remainder, `each`) are global too."""
    def __init__(self, hp, counters, budget_left, used, class_entries, forms, walk_pos=None, iterations=1, drawn=None, status=0, draw_info=None, item_pos=None):
        self._hp, self.mask, self.label = hp, hp.pseudo_mask, hp.pseudo_label
        self.counters, self.budget_left, self._used, self.class_entries, self.forms = counters, budget_left, used, class_entries, forms
        self.walk_pos = walk_pos
        # the seed / random / label-all rounds: iterations run, the items of every iteration (region ids), sampler.ST_MAX_ITER when max_iter stopped the loop
        # draw_info: per iteration dict(live, k, items, remain, each) — the live clouds, the clicks drawn for, the items, the seed remainder, each_file_number
        # sharded: `drawn` are this rank's items per iteration (local region ids), `item_pos` their places in the union's item list, `walk_pos` the used
        # regions' walk positions, both per iteration: enough to merge the ranks' results into the single process's order; the rest is global
        self.iterations, self.drawn, self.status, self.draw_info, self.item_pos = int(iterations), drawn, int(status), draw_info, item_pos

    @property
    def used(self):
        return self._used.tolist()

    def to_host(self, cloud=None):
        """pseudo_gt as io_formats.save_gt writes it: float32 [2, n_c] of one cloud (None: [2, n] over all points)"""
        both = np.stack([self.mask.to_host(self._hp.sel_stream), self.label.to_host(self._hp.sel_stream)])
        if cloud is None:
            return both
        if self._hp.pt_off is None:
            raise ValueError("to_host(cloud): the HotPath does not know where its clouds' points start (set pt_off)")
        return np.ascontiguousarray(both[:, int(self._hp.pt_off[cloud]): int(self._hp.pt_off[cloud + 1])])


class _Rows:
    """rows [lo, hi) of a DevArray's first axis with the surface the stages use (ptr / shape / dtype / to_host): the batches of an AL round write
    their tiles and network outputs straight into their slice of the round's arrays"""
    def __init__(self, arr, lo, hi):
        rowb = arr.dtype.itemsize * int(np.prod(arr.shape[1:], dtype=np.int64))
        self.base, self.dtype, self.shape = arr, arr.dtype, (int(hi - lo),) + tuple(arr.shape[1:])
        self.ptr, self.nbytes = int(arr.ptr) + int(lo) * rowb, int(hi - lo) * rowb

    def to_host(self, stream=None):
        out = np.empty(self.shape, self.dtype)
        if stream is None:
            _lib.check(_lib.lib().ssdr_memcpy_d2h(_lib.ptr(out), self.ptr, self.nbytes))
        else:
            _lib.check(_lib.lib().ssdr_memcpy_d2h_on(_lib.ptr(out), self.ptr, self.nbytes, stream))
        return out


class ALRound:
    """ONE active-learning round at the reference's own scale: the network runs over ALL clouds of the pool and then ONE selection picks
    `batch_size` regions among 2 x batch_size candidates (+ the labelled rows) of all of them (ssdr_main_S3DIS2.py:134: 10 000 regions per round;
    sampler2.py:580-642 prediction over every cloud, :736-781 one GCN_FPS_sampling).  bench.py's step selects per 16-tile batch instead, which
    keeps the reference's picks-per-tile ratio but under-represents the quadratic term of the farthest-point chain 17-fold; this class is the
    round as the reference runs it: `n_batches` batches of len(rooms) tiles go through front end -> KNN pyramid -> inference (three streams, three
    buffer sets, batches overlapped), their tiles / labels / probabilities / features land in the round's arrays, then scoring over all points and
    the one-call device chain (ssdr_gcn_fps_sampling_dev) over all clouds' regions.  Tiles of batch b are cut from the same raw rooms with the
    randomness of room id b * len(rooms) + i (another pick point, shuffle and padding draw: another tile).
    comm: a sharded round.  A rank owns a contiguous share of the batches (np.array_split over the ranks; uneven shares are allowed, a rank without a
    batch is refused), allocates and infers only those, and keeps their GLOBAL tile ids for the randomness, the labelled stand-in and room_ids: the union
    of the ranks' tiles is the single-process round's.  run() and label() then pass the communicator on to the scoring, the selection and the oracle."""
    SLOTS = 4          # batches in flight = HIP streams = the runtime's hardware queues (2: 54.9 ms for 17 batches, 3: 52.2, 4: 49.1, 5: 56.9, 6: 49.4, 8: 49.6; a stream per STAGE: 60-64)

    def __init__(self, weights, rooms, n_batches, config=ConfigS3DIS, batch_size=10000, round_num=5, labeled_per_tile=15, precision="f32",
                 selector="fps", tiles32=True, seed=0, gcn_number=1, gcn_top=0, min_size=1, gcn_steps=20000, gcn_dropout=0.3, gcn_seed=0, gcn_form="auto", comm=None,
                 draws="device", draw_seed=0, max_iter=32):
        L = _lib.lib()
        self.comm = comm
        draw_kw = dict(draws=draws, draw_seed=draw_seed, max_iter=max_iter)      # the seed / random / label-all samplers' draws (HotPath)
        self.batch_ids = list(range(int(n_batches)))          # the global ids of this process's batches
        if comm is not None:
            if selector == "coregcn":
                raise ValueError('selector="coregcn" with a communicator: the sharded form of the trained-GCN selector is not offered')
            if selector in REGION_SAMPLERS:
                _region_check_comm(selector, comm, draws)
            if comm.world > int(n_batches):                   # (raised on every rank: nobody is left waiting in an exchange)
                raise ValueError("ALRound: %d batches cannot be shared among %d ranks (a rank would own none)" % (int(n_batches), comm.world))
            self.batch_ids = [int(b) for b in np.array_split(np.arange(int(n_batches)), comm.world)[comm.rank]]
        self.cfg, self.nb, self.B, self.rooms = config, len(self.batch_ids), len(rooms), rooms
        N = config.num_points
        self.tiles = self.nb * self.B
        # One stream per stage.  A consumer stage waits for "everything its producer stream holds so far" (ssdr_stream_wait), which names exactly its own
        # batch because a step enqueues consumer first (inference k - 2, pyramid k - 1, front end k); the front end's wait for the LAST READER of the buffer
        # set it reuses (inference k - SLOTS) is an event recorded behind that inference (ssdr_event_*): with three buffer sets and a stream-wide wait the
        # front end ran at most two batches ahead and the 17 batches took 60 ms; five sets and the event: the stages run as far ahead as their inputs allow.
        self.streams = [_new_stream() for _ in range(3)]
        self.s_front, self.s_knn, self.s_inf = self.streams
        self.SLOTS = int(os.environ.get("SSDR_AL_SLOTS", self.SLOTS))
        self.bstreams = [_new_stream() for _ in range(self.SLOTS)]
        self.ev_inf = []
        for _ in range(self.nb):
            e = C.c_void_p(); _lib.check(L.ssdr_event_create(C.byref(e))); self.ev_inf.append(e.value)
        s_i = self.s_inf
        self.work = []
        for w in range(self.SLOTS):
            h = HotPath(weights, config, precision=precision, tiles32=tiles32, seed=seed, select_per_tile=1, labeled_per_tile=1)
            h.front_stream, h.knn_stream, h.stream, h.pipelined = self.s_front, self.s_knn, s_i, True
            h.load_rooms(rooms, list(range(self.B)))
            self.work.append(h)
        P = self.tiles * N
        self.xyz = DevArray((P, 3), np.float32); self.tile_l = DevArray((P,), np.int32)
        self.probs = DevArray((P, config.num_classes), np.float32); self.f32 = DevArray((P, 32), np.float32)
        # per batch: the tiles' randomness and where its outputs go
        self.batches = []
        h0 = self.work[0]
        for b in range(self.nb):
            draws = [h0.draw_room(r[0], self.batch_ids[b] * self.B + i) for i, r in enumerate(rooms)]
            lo, hi = b * self.B * N, (b + 1) * self.B * N
            self.batches.append(dict(centers=np.ascontiguousarray(np.stack([d["center"] for d in draws]), np.float32),
                                     perm=DevArray.from_host(np.stack([d["perm"] for d in draws])), dup=DevArray.from_host(np.stack([d["dup"] for d in draws])),
                                     xyz=_Rows(self.xyz, lo, hi), tile_l=_Rows(self.tile_l, lo, hi), probs=_Rows(self.probs, lo, hi), f32=_Rows(self.f32, lo, hi)))
        # setup (untimed): every batch's tiles once, their superpoints (stand-in for the partition, as HotPath.load_rooms), the labelled stand-in
        for b in range(self.nb):
            self._bind(b)._front_end()
        _lib.sync(self.s_front)
        _lib.check(L.ssdr_grid_subsample_status(self.s_front, None))
        tiles = self.xyz.to_host().reshape(self.tiles, N, 3)
        offs, pts, cloud, labeled = [np.zeros(1, np.int64)], [], [], {}
        tile_ids = [bg * self.B + i for bg in self.batch_ids for i in range(self.B)]      # global tile ids (a sharded round: this rank's)
        for t in range(self.tiles):
            o, p = synthetic.superpoints_from_tile(tiles[t])
            base = int(sum(len(x) for x in cloud))
            pts.append(p.astype(np.int64) + t * N); offs.append(o[1:].astype(np.int64) + offs[-1][-1]); cloud.append(np.full(len(o) - 1, t, np.int32))
            rng = np.random.default_rng([seed, tile_ids[t], 1])
            n_sp = len(o) - 1
            labeled[t] = set((base + rng.choice(n_sp, min(labeled_per_tile, n_sp), replace=False)).tolist())
        sel_list = np.random.default_rng([seed, 999983]).integers(0, config.num_classes, 4000)
        self.sel = HotPath.from_device(self.xyz, self.probs, self.f32, self.tile_l, np.concatenate(offs), np.concatenate(pts), np.concatenate(cloud), labeled, sel_list,
                                       config, room_ids=tile_ids, batch_size=batch_size, round_num=round_num, selector=selector, gcn_number=gcn_number, gcn_top=gcn_top, min_size=min_size, seed=seed,
                                       gcn_steps=gcn_steps, gcn_dropout=gcn_dropout, gcn_seed=gcn_seed, gcn_form=gcn_form, **draw_kw)
        self.sel.stream = self.sel.score_stream = self.sel.sel_stream = s_i
        self.sel.front_stream = s_i; self.sel.pipelined = True
        self.sel.pt_off = np.arange(self.tiles + 1, dtype=np.int64) * N
        self.tile_points = P

    def _bind(self, b):
        """worker of batch b with the batch's randomness and output slices"""
        h, d = self.work[b % self.SLOTS], self.batches[b]
        h.centers, h.perm, h.dup = d["centers"], d["perm"], d["dup"]
        h.xyz, h.tile_l, h.probs, h.f32 = d["xyz"], d["tile_l"], d["probs"], d["f32"]
        return h

    def infer_all(self):
        """front end -> KNN pyramid -> inference of every batch, enqueued.  A BATCH PER STREAM (default): batch b runs its three stages in order on stream
        b mod SLOTS, whose previous batch used the same buffer set — no cross-stream wait at all, and what overlaps is whatever the SLOTS batches in flight
        have to offer each other (a pyramid's latency-bound tree hand-over beside the next batch's grid search as well as beside another stage).
        SSDR_AL_SCHED=stage: a stream per stage with producer waits and an event for the buffer set's last reader (measured slower, tools/al_probe.py)."""
        L = _lib.lib()
        if os.environ.get("SSDR_AL_SCHED", "batch") == "batch":
            for b in range(self.nb):
                h = self._bind(b)
                st = self.bstreams[b % self.SLOTS]
                h.front_stream = h.knn_stream = h.stream = st
                if b < self.SLOTS:
                    _lib.check(L.ssdr_stream_wait(st, self.s_inf))      # (the previous round's selection, which read these arrays, has finished)
                h._front_end(); h._pyramid(); h._infer()
            for st in self.bstreams[: min(self.SLOTS, self.nb)]:
                _lib.check(L.ssdr_stream_wait(self.s_inf, st))          # the selection (on the inference stream) starts after every batch
            return
        s_f, s_k, s_i = self.s_front, self.s_knn, self.s_inf
        nowait = bool(os.environ.get("SSDR_AL_NOSLOTWAIT"))       # (development, timing only: a front end may then overwrite buffers an inference still reads)
        _lib.check(L.ssdr_stream_wait(s_f, s_i))                  # (a previous round's inferences, and the selection that read their outputs, have finished)
        for k in range(self.nb + 2):
            if 0 <= k - 2 < self.nb:
                h = self._bind(k - 2); h.stream = s_i
                _lib.check(L.ssdr_stream_wait(s_i, s_k))          # (the pyramid stream's newest work is batch k - 2's)
                h._infer()
                _lib.check(L.ssdr_event_record(self.ev_inf[k - 2], s_i))
            if 0 <= k - 1 < self.nb:
                h = self._bind(k - 1); h.knn_stream = s_k
                _lib.check(L.ssdr_stream_wait(s_k, s_f))          # (the front stream's newest work is batch k - 1's)
                h._pyramid()
            if k < self.nb:
                h = self._bind(k); h.front_stream = s_f
                if k >= self.SLOTS and not nowait:                # the buffer set's last reader: the inference of batch k - SLOTS
                    _lib.check(L.ssdr_stream_wait_event(s_f, self.ev_inf[k - self.SLOTS]))
                h._front_end()

    def run(self):
        """the whole round; returns (picked candidate indices, candidate list) as HotPath.step does"""
        if self.sel.selector in REGION_SAMPLERS:      # RandomSampler / AllSampler look at no network output: no inference, no scoring
            return self.sel.step_selection(self.comm)
        self.infer_all()
        self.sel._score_async(self.comm)
        self.sel._select_issue(self.comm)
        out = self.sel._select_collect()
        for st in [self.s_knn] + self.bstreams:
            knn.knn_status(st)
            _lib.check(_lib.lib().ssdr_grid_subsample_status(st, None))
        _lib.check(_lib.lib().ssdr_grid_subsample_status(self.s_front, None))
        return out

    def label(self, mode="NAIL", threshold=0.9, min_size=None, budget=None):
        """the oracle over the round's picks (HotPath.label_selected on the round's arrays): the labelled set, the class list and the pseudo labels
        are then those of the next round"""
        return self.sel.label_selected(mode=mode, threshold=threshold, min_size=min_size, budget=budget, comm=self.comm)

    def seed(self, number, round_num=0):
        """SeedSampler over the round's regions (HotPath.seed_round): the labelled set every experiment starts from, in place of the labelled stand-in;
        a sharded round seeds over all ranks' regions with its communicator"""
        return self.sel.seed_round(number, round_num, comm=self.comm)


class BatchStreams:
    """`slots` batches in flight, A BATCH PER STREAM: batch k runs front end -> KNN pyramid -> network -> scoring -> selection in order on stream
    k mod slots, on the buffer set that stream's previous batch used.  No cross-stream wait exists; what overlaps is whatever the batches in flight
    have to offer each other (a selection's one-workgroup chain beside another batch's network, a pyramid's tree hand-over beside a front end).
    Against Pipelined (a stream per STAGE) there is no fill — every stream is busy from the first launch on — and the drain is the last batches'
    selections; the host waits for the selection of batch k - slots before it reuses its buffers.  Same interface as Pipelined for bench.py."""

    def __init__(self, make_hot_path, slots=4, sel_streams=0):
        """sel_streams > 0: the selections run on that many streams of their own, taken in turn (a selection waits for its batch's stream; the batch's
        stream goes on to its next batch only after the host has read that selection: the buffer set is the same)"""
        self.depth = self.slots = int(slots)
        self.streams = [_new_stream() for _ in range(self.slots)]
        self.sel_streams = [_new_stream() for _ in range(int(sel_streams))]
        self.hp = [make_hot_path() for _ in range(self.slots)]
        for h, st in zip(self.hp, self.streams):
            h.pipelined = True
            h.front_stream = h.knn_stream = h.stream = h.score_stream = h.sel_stream = st
        self._issued = []
        self._k = 0
        self.finish()

    def run(self, steps, comm=None, steady=False):
        """finishes `steps` selections (every batch issued is completed before the call returns)"""
        out = None
        for k in range(steps):
            h = self.hp[k % self.slots]
            if len(self._issued) >= self.slots:              # the buffer set's previous batch: its result is read before the set is reused
                out = self._issued.pop(0)._select_collect()
            h._front_end(); h._pyramid(); h._infer(); h._score_async(comm)
            if self.sel_streams:
                h.sel_stream = self.sel_streams[self._k % len(self.sel_streams)]
                _lib.check(_lib.lib().ssdr_stream_wait(h.sel_stream, h.stream))
            h._select_issue(comm)
            self._issued.append(h); self._k += 1
        while self._issued:
            out = self._issued.pop(0)._select_collect()
        return out

    def finish(self):
        while self._issued:
            self._issued.pop(0)._select_collect()
        _lib.sync()
        for st in self.streams + self.sel_streams:
            _lib.sync(st)
        for st in self.streams:
            knn.knn_status(st)
            _lib.check(_lib.lib().ssdr_grid_subsample_status(st, None))


class _Prefix:
    """the first `count` elements of a DevArray as a flat array of its own (exchange buffers)"""
    def __init__(self, arr, count):
        self.base = arr          # (the buffer stays the array's: a prefix that outlived it would point into the pool of freed buffers)
        self.ptr, self.dtype, self.shape, self.nbytes = arr.ptr, arr.dtype, (int(count),), int(count) * arr.dtype.itemsize
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": self.dtype.str, "data": (int(self.ptr), False), "version": 2, "strides": None}

    def host_view(self):
        return np.frombuffer((C.c_char * self.nbytes).from_address(int(self.ptr)), self.dtype)


class Pipelined:
    """Overlap consecutive batches on separate buffer sets and HIP streams (software pipeline over the stages
    front end | KNN pyramid | network | scoring | selection).  `depth` batches are in flight:
    depth 2: selection of batch k (latency-bound: host decisions, one workgroup of FPS) on the main stream next to
             everything else of batch k+1 on a second stream;
    depth 3: front end (subsample + tiles) on its own stream, one batch further ahead;
    depth 4: front end + KNN pyramid | network | scoring | selection — three created streams + the main one; the choice when a
             framework's own streams (RCCL exchanges) share the process and its 4 hardware queues (92 vs 63 Mpoints/s);
    depth 5 (default): every stage on its own stream (one GPU, no framework streams: 99 vs 86 Mpoints/s for depth 4).
    Every batch still goes through every stage; `run(K)` finishes K selections."""
    STAGES = ("front", "knn", "infer", "score")
    GROUPS = {2: (0, 0, 0, 0), 3: (0, 1, 1, 1), 4: (0, 0, 1, 2), 5: (0, 1, 2, 3)}     # stage -> stream group

    def __init__(self, make_hot_path, depth=5, groups=None, overlap_select=True, sel_lag=1, spare_set=False):
        """groups: optional stage -> stream-group tuple for (front, knn, infer, score), non-decreasing from 0; depth = last group + 2"""
        if groups is not None:
            depth = groups[-1] + 2
        assert groups is not None or depth in self.GROUPS
        self.depth = depth
        self.group = dict(zip(self.STAGES, groups if groups is not None else self.GROUPS[depth]))
        # The runtime spreads the streams over its (4) hardware queues in the order they are created, after the NULL stream and the
        # library's own (both brought into use by ssdr_init); streams that share a queue serialise.  Which stage shares with which decides
        # the overlap: measured on MI355X / ROCm 7.2 at depth 5 with one unused stream created in front of the stage streams 4.8 ms per
        # step, without it 6.4, with two 6.1, with three 5.3, with the unused one in any later position 5.7-6.2 (`GPU_MAX_HW_QUEUES=8`, every
        # stream on a queue of its own: 4.8 as well).  So: one spare in front.
        qmap = os.environ.get("SSDR_PIPE_QMAP")              # development: "f,k,i,s,a,b" = the hardware queue (1..GPU_MAX_HW_QUEUES) wanted for the front / knn / infer /
        if qmap and depth == 5 and overlap_select:           # score streams and the two selection streams ("-" for a: the library stream, queue 1)
            # ROCm 7.2's runtime (read off rocprofv3's queue ids, tools/gpu_qdiscover.sh): the library's stream holds queue 1, the NULL stream queue 2, every new stream
            # opens a new queue until GPU_MAX_HW_QUEUES (4) exist and then joins the queue with the fewest streams, the HIGHEST id among equals; unused streams count
            want = qmap.split(",")
            maxq = int(os.environ.get("GPU_MAX_HW_QUEUES") or 4)
            refs = {1: 1, 2: 1}
            self._spares = []

            def next_queue():
                if len(refs) < maxq:
                    return len(refs) + 1
                low = min(refs.values())
                return max(q for q, r in refs.items() if r == low)

            def on_queue(q):
                q = int(q)
                for _ in range(64):
                    nq = next_queue()
                    refs[nq] = refs.get(nq, 0) + 1
                    st = _new_stream()
                    if nq == q:
                        return st
                    self._spares.append(st)
                raise RuntimeError("SSDR_PIPE_QMAP: queue %d not reachable" % q)
            made = []                                       # creation in the order given: front, knn, infer, score, selA, selB
            for i in range(6):
                made.append(None if want[i] == "-" else on_queue(want[i]))
            self.streams, self.sel_streams = made[:4], made[4:]
            self._spare = None
        else:
            self._spare = _new_stream()
            self.streams = [_new_stream() for _ in range(depth - 1)]
            self.sel_streams = [None]                        # selections alternate between the library stream and one of their own
            if overlap_select:
                self.sel_streams.append(_new_stream())
        self.overlap_select = overlap_select
        # sel_lag: how many selections behind the newest the host waits for (1: the previous batch's).  The sharded run's replicated global FPS
        # grows with the square of the rank count: from 4 ranks on a chain is longer than two steps, and sel_lag = 2 keeps
        # three chains in flight on three streams, with one more buffer set so that no stage overwrites what a running selection reads
        self.sel_lag = max(1, int(sel_lag)) if overlap_select else 1
        for _ in range(self.sel_lag - 1):
            self.sel_streams.append(_new_stream())
        self._issued = []                                    # selections enqueued, not collected yet (oldest first)
        self.lead = {n: depth - 1 - g for n, g in self.group.items()}      # batches ahead of the selection
        # one buffer set per batch in flight (a spare set, so that no stage has to wait for the previous selection's buffers, was
        # measured slower: 127 vs 137 Mpoints/s — a sixth working set in the caches costs more than the deferred front end)
        self.slots = depth + self.sel_lag - 1 + (1 if spare_set else 0)      # spare_set: nothing is deferred behind the wait for the previous selection
        self.hp = [make_hot_path() for _ in range(self.slots)]
        for h in self.hp:
            h.pipelined = True
            h.front_stream, h.knn_stream = self.streams[self.group["front"]], self.streams[self.group["knn"]]
            h.stream, h.score_stream = self.streams[self.group["infer"]], self.streams[self.group["score"]]
        self._k = 0
        self._drain()

    def _drain(self):
        _lib.sync()
        for st in self.streams + [x for x in self.sel_streams if x is not None]:
            _lib.sync(st)

    def _stage(self, name, b):
        """enqueue one stage of batch b; a consumer stream first waits for everything its producer stream holds so far"""
        h = self.hp[b % self.slots]
        i = self.STAGES.index(name)
        if i > 0 and self.group[name] != self.group[self.STAGES[i - 1]]:
            _lib.check(_lib.lib().ssdr_stream_wait(self.streams[self.group[name]], self.streams[self.group[self.STAGES[i - 1]]]))
        if name == "score":
            h._score_async(self.comm)
        else:
            {"front": h._front_end, "knn": h._pyramid, "infer": h._infer}[name]()

    def run(self, steps, comm=None, steady=False):
        """Finishes `steps` selections.  steady=False: fills the pipe, runs, drains (every issued batch is completed).
        steady=True keeps the pipe full across calls: the first call fills it, and every later step issues exactly one launch sequence
        of EVERY stage (on consecutive batches) and completes one selection — what bench.py times; finish() drains.

        The selection chain (host decisions, ~3 ms of dependent launches ending in the one-workgroup FPS) is the longest stage and the only
        one the host waits for.  With overlap_select the host enqueues the selection of batch k, then the other stages, and only then
        waits for the selection of batch k - 1 (alternating selection streams): the chains of consecutive batches overlap and the step
        is no longer the latency of one chain.  The stage that reuses the buffer set of batch k - 1 is enqueued after that wait."""
        self.comm = comm
        L = _lib.lib()
        out = None
        lead, first = self.lead, self.lead["front"]
        k0 = self._k if steady else 0
        last = None if steady else steps                     # batches >= last are never issued
        if k0 == 0:
            self._issued = []
            for b in range(first if steady else min(steps, first)):      # prologue: fill the pipe
                for name in self.STAGES:
                    if b < lead[name]:
                        self._stage(name, b)
        for k in range(k0, k0 + steps):
            hk = self.hp[k % self.slots]
            hk.sel_stream = self.sel_streams[k % len(self.sel_streams)] if self.overlap_select else None
            _lib.check(L.ssdr_stream_wait(hk.sel_stream, self.streams[self.group["score"]]))    # selection stream: batch k's scores are ready
            hk._select_issue(comm)                           # batch k: host decisions + the whole selection chain enqueued ...
            deferred = []
            for b in range(k + 1, k + first + 1):            # ... the other stages are issued while its FPS chain (one workgroup,
                if last is not None and b >= last:           # ~1.4 ms) runs, instead of before it ...
                    break
                for name in self.STAGES:
                    if b == k + lead[name]:
                        if self.overlap_select and b - k == self.slots - self.sel_lag:      # (never with a spare set: b - k < depth)
                            deferred.append((name, b))       # writes the buffer set of batch k - sel_lag, whose selection may still run
                        else:
                            self._stage(name, b)             # the buffer set of batch b was last read by select(b - depth), done
            if self.overlap_select:
                self._issued.append(k)
                while len(self._issued) > self.sel_lag:
                    out = self.hp[self._issued.pop(0) % self.slots]._select_collect()
                for name, b in deferred:
                    self._stage(name, b)
            else:
                out = hk._select_collect()                   # ... and only then the host waits for the selection
        if steady:
            self._k = k0 + steps
            if out is None and self._issued:                       # a short call right after the fill: nothing older to hand back
                while self._issued:
                    out = self.hp[self._issued.pop(0) % self.slots]._select_collect()
        else:
            while self.overlap_select and self._issued:
                out = self.hp[self._issued.pop(0) % self.slots]._select_collect()
            self._drain()
        return out

    def finish(self):
        """end a steady run: wait for everything issued and forget the partially processed batches"""
        while self._issued:
            self.hp[self._issued.pop(0) % self.slots]._select_collect()
        self._drain()
        knn.knn_status(self.streams[self.group["knn"]])     # everything has finished: the blocking checks
        _lib.check(_lib.lib().ssdr_grid_subsample_status(self.streams[self.group["front"]], None))
        self._k = 0
