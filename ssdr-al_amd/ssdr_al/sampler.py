"""Host-side mirror of the numeric part of the reference's selection code
(/root/reference/SSDR_AL_s3dis/sampler2.py, fps_gcn_cpu.py, kcenterGreedy.py): same function names and argument
meaning where the reference has a function, arrays instead of pickles/PLY files (file I/O is out of scope).
Every computation runs in libssdr_al.so; this module only moves arrays and sequences the calls.

Superpoints are passed as CSR (offsets int32 [S+1], points int32 [T]); ``csr_from_components`` converts the
reference's ``components`` object array (partition/compute_superpoint.py:63-68)."""
import numpy as np

from . import _lib
from ._lib import DevArray

_UNC = {"lc": 0, "entropy": 1, "sb": 2}
_REG = {"mean": 0, "sum_weight": 1, "WetSU": 2}


def _mode(sampler_args, table):
    for k in table:                       # the reference tests `"lc" in sampler_args` etc. in this order
        if k in sampler_args:
            return table[k]
    raise ValueError("no known mode in %r" % (sampler_args,))


def csr_from_components(components):
    sizes = np.array([len(c) for c in components], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pts = np.concatenate([np.asarray(c, np.int32) for c in components]) if len(components) else np.zeros(0, np.int32)
    return off, pts.astype(np.int32)


def compute_point_uncertainty(prob_logits, sampler_args, return_class=False):
    """sampler2.py:28-47 (+ np.argmax of :602 when return_class)."""
    prob = np.ascontiguousarray(prob_logits, np.float32)
    n, C = prob.shape
    d_p = DevArray.from_host(prob); d_u = DevArray((n,), np.float32); d_c = DevArray((n,), np.int32)
    _lib.check(_lib.lib().ssdr_point_uncertainty_dev(d_p.ptr, n, C, _mode(sampler_args, _UNC), d_u.ptr, d_c.ptr, None))
    _lib.sync()
    return (d_u.to_host(), d_c.to_host()) if return_class else d_u.to_host()


def compute_region_stats(pixel_uncertainty, pixel_class, offsets, points, class_num, sampler_args):
    """The per-superpoint loop of TSampler.prediction (sampler2.py:612-626) for one cloud:
    region uncertainty (compute_region_uncertainty :12-26), dominant class (_dominant_label :102-106) and the
    number of dominant-class members (_dominant_2 :108-115)."""
    S = len(offsets) - 1
    d_u = DevArray.from_host(np.ascontiguousarray(pixel_uncertainty, np.float32))
    d_c = DevArray.from_host(np.ascontiguousarray(pixel_class, np.int32))
    d_o = DevArray.from_host(np.ascontiguousarray(offsets, np.int32)); d_p = DevArray.from_host(np.ascontiguousarray(points, np.int32))
    d_r = DevArray((S,), np.float64); d_d = DevArray((S,), np.int32); d_n = DevArray((S,), np.int32)
    _lib.check(_lib.lib().ssdr_region_stats_dev(d_u.ptr, d_c.ptr, d_o.ptr, d_p.ptr, S, class_num, _mode(sampler_args, _REG),
                                                d_r.ptr, d_d.ptr, d_n.ptr, None))
    _lib.sync()
    return d_r.to_host(), d_d.to_host(), d_n.to_host()


def dominant_labels(labels, offsets, points, num_labels):
    """ssdr_max_dominant / oracle_labeling "dominant" (sampler2.py:102-106, :127-144): label and purity per superpoint."""
    S = len(offsets) - 1
    d_l = DevArray.from_host(np.ascontiguousarray(labels, np.int32))
    d_o = DevArray.from_host(np.ascontiguousarray(offsets, np.int32)); d_p = DevArray.from_host(np.ascontiguousarray(points, np.int32))
    d_lab = DevArray((S,), np.int32); d_pur = DevArray((S,), np.float64)
    _lib.check(_lib.lib().ssdr_dominant_label_dev(d_l.ptr, d_o.ptr, d_p.ptr, S, num_labels, d_lab.ptr, d_pur.ptr, None))
    _lib.sync()
    return d_lab.to_host(), d_pur.to_host()


LABEL_COUNTERS = ("sp_num", "p_num", "sub_num", "sub_p_num", "split_sp_num", "ignore_sp_num")
LABEL_STATUS = ((1, "a ground-truth label outside [0, num_labels)"), (2, "a predicted class outside [0, num_classes)"),
                (4, "a region or point id outside the arrays"), (8, "more class entries than the class list holds"))


def label_mode(sampler_args):
    """the oracle mode a reference `sampler_args` names, tested in the reference's order (sampler2.py:127, :146); -1: none (the library refuses it)"""
    args = [sampler_args] if isinstance(sampler_args, str) else list(sampler_args)
    return 0 if "dominant" in args else 1 if "NAIL" in args else -1


def label_status_check(status):
    if status:
        raise ValueError("oracle_label: " + "; ".join(msg for bit, msg in LABEL_STATUS if status & bit) + " (status %d)" % status)


def oracle_labeling(superpoint_inds, components, input_gt, pseudo_gt, cloud_name, w, sampler_args, prob_class, threshold, budget, min_size, total_obj,
                    num_labels=64, num_classes=32):
    """sampler2.py:124-192 for one cloud through ssdr_oracle_label_dev: walks `superpoint_inds` while budget["click"] lasts, writes the two rows of
    `pseudo_gt` ([2, n]: labelled flag, pseudo label), appends to total_obj["selected_class_list"], adds to the counters in `w`, takes the clicks from
    `budget`; returns (pseudo_gt, used_superpoint_inds).  sampler_args names the mode ("dominant" or "NAIL"); prob_class [n] are the predicted classes
    (NAIL).  Labels go up to num_labels - 1 <= 63, classes up to num_classes - 1 <= 31."""
    inds = np.asarray(list(superpoint_inds), np.int64).reshape(-1)
    off, pts = csr_from_components(components)
    gt = np.ascontiguousarray(np.asarray(input_gt).reshape(-1), np.int32)
    n, S, M = len(gt), len(off) - 1, len(inds)
    mode = label_mode(sampler_args)
    m0 = np.ascontiguousarray(np.asarray(pseudo_gt[0]), np.float32); l0 = np.ascontiguousarray(np.asarray(pseudo_gt[1]), np.float32)
    d_gt = DevArray.from_host(gt)
    d_pred = None if prob_class is None else DevArray.from_host(np.ascontiguousarray(np.asarray(prob_class).reshape(-1), np.int32))
    d_off, d_pts = DevArray.from_host(off), DevArray.from_host(pts)
    d_cloud = DevArray.from_host(np.zeros(max(S, 1), np.int32))
    d_items = DevArray.from_host(np.concatenate([inds, [0]]).astype(np.int32)); d_n = DevArray.from_host(np.array([M], np.int32))
    d_budget = DevArray.from_host(np.array([int(budget["click"])], np.int64))
    d_m, d_l = DevArray.from_host(m0), DevArray.from_host(l0)
    d_used = DevArray((max(M, 1),), np.uint8); d_lab = DevArray.from_host(np.zeros(max(S, 1), np.uint8))
    cap = max(1, min(M * 32, max(int(budget["click"]), 0) + 33))
    d_cls = DevArray((cap,), np.int32); d_out = DevArray((12,), np.int64)
    _lib.check(_lib.lib().ssdr_oracle_label_dev(d_gt.ptr, d_pred.ptr if d_pred is not None else None, n, d_off.ptr, d_pts.ptr, S, d_cloud.ptr, 1, d_items.ptr,
                                                d_n.ptr, M, None, int(np.diff(off).max()) if S else 1, int(num_labels), int(num_classes), mode, float(threshold),
                                                int(min_size), d_budget.ptr, d_m.ptr, d_l.ptr, d_used.ptr, d_lab.ptr, d_cls.ptr, cap, None, d_out.ptr, None))
    _lib.sync()
    out = d_out.to_host()
    label_status_check(int(out[8]))
    m1, l1 = d_m.to_host(), d_l.to_host()
    ch = np.flatnonzero((m1 != m0) | (l1 != l0))          # (points the walk did not write keep the caller's values, whatever their type)
    pseudo_gt[0][ch] = m1[ch]; pseudo_gt[1][ch] = l1[ch]
    for k, name in enumerate(LABEL_COUNTERS):
        if out[k] or name in w:
            w[name] = w.get(name, 0) + int(out[k])
    budget["click"] = int(out[7])
    total_obj.setdefault("selected_class_list", []).extend(d_cls.to_host()[: int(out[6])].tolist())
    used = d_used.to_host()[:M]
    return pseudo_gt, [superpoint_inds[i] for i in np.flatnonzero(used)]


# ---- the seed, random and label-all samplers (sampler2.py:344-520): csrc/select_random.hip ------------------------------------------------------
REGION_RANDOM, REGION_ALL = 0, 1
DRAW_ST_COUNT, DRAW_ST_ITEMS, DRAW_ST_CLOUD = 1, 2, 4
ST_MAX_ITER = 256          # LabelResult.status: the loop stopped after max_iter iterations (the reference recurses for ever there)


def _iteration_draws(total_num, unlabeled, number, random_state):
    """The draws of one SeedSampler._iteration / RandomSampler._iteration (sampler2.py:357-379, :465-486), consuming `random_state` exactly as the
    reference consumes np.random: unlabeled = {cloud: [region, ...]} in the reference's dict and list order.
    -> ([(cloud, [region, ...])] in the order _help is called, each_file_number, the seed remainder)"""
    rand_inds = random_state.choice(np.arange(int(total_num)), int(number), replace=False)
    names = list(unlabeled)
    length = len(names)
    each_file_number = np.zeros([length], dtype=np.int32)
    for ind in rand_inds:
        each_file_number[ind % length] += 1
    picks, remain = [], 0
    for i in range(length):
        if each_file_number[i] > 0:
            unl = unlabeled[names[i]]
            if len(unl) >= each_file_number[i]:
                inds = random_state.choice(list(unl), int(each_file_number[i]), replace=False).tolist()
            else:
                inds = list(unl)
                remain += int(each_file_number[i]) - len(inds)
            picks.append((names[i], inds))
    return picks, each_file_number, remain


def random_iteration_host(total_num, unlabeled, click, random_state):
    """RandomSampler._iteration's draws for budget["click"] = click -> (picks, each_file_number)"""
    picks, each, _ = _iteration_draws(total_num, unlabeled, click, random_state)
    return picks, each


def seed_iteration_host(total_num, unlabeled, number, random_state):
    """SeedSampler._iteration's draws -> (picks, each_file_number, remain_number)"""
    return _iteration_draws(total_num, unlabeled, number, random_state)


def remove_used(unlabeled, cloud, used):
    """what _help / _help_seed leave of a cloud's list (sampler2.py:214-216), that expression's order included"""
    unlabeled[cloud] = list(set(unlabeled[cloud]) - set(used))
    if len(unlabeled[cloud]) == 0:
        del unlabeled[cloud]


def region_draw_status_check(status, k=None, total_num=None):
    if status & DRAW_ST_COUNT:
        raise ValueError("Cannot take a larger sample than population when 'replace=False' (%s clicks of total_num = %s)" % (k, total_num))
    if status & DRAW_ST_ITEMS:
        raise RuntimeError("region_draw: more items than the item list holds")
    if status & DRAW_ST_CLOUD:
        raise ValueError("region_draw: a region's cloud is outside the cloud table")


def add_clsbal(class_num, region_class, region_uncertainty, total_obj, skip=None):
    """sampler2.py:262-266.  The reference passes the UNLABELLED regions only (prediction(), :612-627); a caller that keeps every region in
    one array marks the others in `skip` (non-zero: not part of the population)."""
    rc = np.ascontiguousarray(region_class, np.int32)
    sel = np.ascontiguousarray(total_obj.get("selected_class_list", []), np.int32)
    d_rc = DevArray.from_host(rc); d_sel = DevArray.from_host(sel) if len(sel) else None
    d_skip = None if skip is None else DevArray.from_host(np.ascontiguousarray(skip).astype(np.uint8))
    d_u = DevArray.from_host(np.ascontiguousarray(region_uncertainty, np.float64))
    _lib.check(_lib.lib().ssdr_clsbal_dev(d_rc.ptr, len(rc), d_skip.ptr if d_skip else None, d_sel.ptr if d_sel else None, len(sel), d_u.ptr, None))
    _lib.sync()
    return d_u.to_host()


def add_classbal(class_num, region_class, region_uncertainty, skip=None):
    """sampler2.py:256-260 (`--classbal 1`): add_clsbal without the already-selected list."""
    return add_clsbal(class_num, region_class, region_uncertainty, {"selected_class_list": []}, skip)


def labeled_class_weights(dominant_label_list, class_num):
    """The draw probabilities of get_labeled_selection_cloudname_spidx_pointidx (sampler2.py:294-295): weights_percentage of the labelled
    regions' ground-truth dominant labels, normalised.  Host arithmetic on a few thousand integers (it feeds np.random.choice)."""
    lab = np.asarray(dominant_label_list, np.int64)
    dist = np.zeros([class_num])
    for c in lab:                                    # weights_percentage :92-100 as written (float64 counts)
        dist[c] = dist[c] + 1
    dist = dist / len(lab)
    w = dist[lab]
    return w / np.sum(w)


def get_labeled_selection(dominant_label_list, class_num, round_num, random_state=np.random):
    """The class-balanced draw of sampler2.py:294-302 over the labelled regions (given by their ground-truth dominant labels, in the
    reference's order: cloud by cloud as prediction() met them, ascending superpoint id): `(round_num - 1) * 1000` of them at most,
    without replacement, with NumPy's legacy generator exactly as the reference draws.  Returns the drawn positions in draw order."""
    n = len(dominant_label_list)
    batch = min((int(round_num) - 1) * 1000, n)
    if n == 0 or batch <= 0:
        return np.zeros(0, np.int64)
    return np.asarray(random_state.choice(a=n, size=batch, replace=False, p=labeled_class_weights(dominant_label_list, class_num)), np.int64)


def rank_regions(region_uncertainty):
    """sorted_inds = np.argsort(-region_uncertainty) (sampler2.py:640); equal values by ascending index."""
    u = np.ascontiguousarray(region_uncertainty, np.float64)
    d_u = DevArray.from_host(u); d_s = DevArray((len(u),), np.int32)
    _lib.check(_lib.lib().ssdr_rank_regions_dev(d_u.ptr, len(u), d_s.ptr, None))
    _lib.sync()
    return d_s.to_host()


def segment_mean_features(last_second_features, pixel_class, dom, offsets, points, sel=None):
    """compute_features (sampler2.py:333,339): mean feature of the dominant-class members of each superpoint."""
    f = np.ascontiguousarray(last_second_features, np.float32)
    n_sel = len(offsets) - 1 if sel is None else len(sel)
    d_f = DevArray.from_host(f); d_c = DevArray.from_host(np.ascontiguousarray(pixel_class, np.int32))
    d_d = DevArray.from_host(np.ascontiguousarray(dom, np.int32))
    d_o = DevArray.from_host(np.ascontiguousarray(offsets, np.int32)); d_p = DevArray.from_host(np.ascontiguousarray(points, np.int32))
    d_s = None if sel is None else DevArray.from_host(np.ascontiguousarray(sel, np.int32))
    d_out = DevArray((n_sel, f.shape[1]), np.float32)
    _lib.check(_lib.lib().ssdr_segment_mean_features_dev(d_f.ptr, f.shape[1], d_c.ptr, d_d.ptr, d_o.ptr, d_p.ptr,
                                                         d_s.ptr if d_s else None, n_sel, d_out.ptr, None))
    _lib.sync()
    return d_out.to_host()


def set_chamfer_mode(mode):
    """arithmetic of the graph's chamfer term, process-wide: "f64" (S3DIS: fps_gcn_cpu.create_cd, the default) or "f32_cuda" (the Semantic3D code's
    create_cd_cuda: float32 CUDA-kernel values, SSRD_AL_semantic3d/fps_gcn_cuda.py:13-30)"""
    _lib.check(_lib.lib().ssdr_select_set_chamfer_mode({"f64": 0, "f32_cuda": 1}[mode]))


def cloud_graph(xyz, offsets, points, sel, gcn_top=0):
    """One cloud's block of fps_adj_all (fps_gcn_cpu.py:40-117): returns (centres [n,3], cd [n,n], adj [n,n])."""
    xyz = np.ascontiguousarray(xyz, np.float32); sel = np.ascontiguousarray(sel, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int32)
    n = len(sel)
    max_sp = int((offsets[sel + 1] - offsets[sel]).max()) if n else 1
    d_x = DevArray.from_host(xyz); d_o = DevArray.from_host(offsets); d_p = DevArray.from_host(np.ascontiguousarray(points, np.int32))
    d_s = DevArray.from_host(sel)
    d_c = DevArray((n, 3), np.float64); d_dir = DevArray((n, n), np.float64); d_a = DevArray((n, n), np.float64)
    _lib.check(_lib.lib().ssdr_cloud_graph_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, n, max(max_sp, 1), int(gcn_top), d_c.ptr, d_dir.ptr, d_a.ptr, None))
    _lib.sync()
    dirm = d_dir.to_host()
    return d_c.to_host(), dirm + dirm.T, d_a.to_host()


def create_cd(xyz, offsets, points, sel):
    """create_cd (fps_gcn_cpu.py:26-38) for the superpoints `sel` of one cloud (centred on their bbox centres)."""
    return cloud_graph(xyz, offsets, points, sel)[1]


def farthest_features_sample(feature_list, sample_number, start):
    """fps_gcn_cpu.py:119-147; `start` replaces the np.random.randint draw of :133."""
    f = np.ascontiguousarray(feature_list, np.float64)
    d_f = DevArray.from_host(f); d_o = DevArray((sample_number,), np.int32)
    _lib.check(_lib.lib().ssdr_fps_dev(d_f.ptr, f.shape[0], f.shape[1], int(start), sample_number, d_o.ptr, None))
    _lib.check(_lib.lib().ssdr_select_status(None, None))      # (a cooperative launch that was not co-resident is an error, not a result)
    _lib.sync()
    return d_o.to_host()


def farthest_superpoint_sample(xyz, offsets, points, sel, sample_number, trigger_idx):
    """sampler2.py:49-80 (the "edcd" branch) for the superpoints `sel` of one cloud (CSR instead of point lists)."""
    xyz = np.ascontiguousarray(xyz, np.float32); sel = np.ascontiguousarray(sel, np.int32)
    offsets = np.ascontiguousarray(offsets, np.int32)
    n = len(sel)
    d_x = DevArray.from_host(xyz); d_o = DevArray.from_host(offsets); d_p = DevArray.from_host(np.ascontiguousarray(points, np.int32))
    d_s = DevArray.from_host(sel)
    d_c = DevArray((n, 3), np.float64); d_dir = DevArray((n, n), np.float64); d_a = DevArray((n, n), np.float64)
    d_out = DevArray((sample_number,), np.int32)
    L = _lib.lib()
    _lib.check(L.ssdr_cloud_graph_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, n, int((offsets[sel + 1] - offsets[sel]).max()), 0, d_c.ptr, d_dir.ptr, d_a.ptr, None))
    _lib.check(L.ssdr_fps_superpoint_dev(d_c.ptr, d_dir.ptr, n, int(trigger_idx), sample_number, d_out.ptr, None))
    _lib.sync()
    return d_out.to_host()


def create_adj(featuresV, labeled_select_ref, unlabeled_candidate_ref, clouds):
    """gcn.create_adj (gcn.py:116-191) with the on-disk inputs replaced by `clouds` {cloud_name: (xyz [n,3] f32, offsets, points)}; refs are
    lists of {"cloud_name", "sp_idx"} as in the reference, featuresV = concatenate(unlabelled candidates, labelled regions) [N,F] (gcn.py:199).
    Returns (normalised features [N,F] float32, adjacency [N,N] float32) like the reference (which also returns its run time)."""
    f = np.ascontiguousarray(featuresV, np.float32)
    N, F = f.shape
    total_cloud, order = {}, []                 # gcn.py:122-138
    for i, r in enumerate(list(unlabeled_candidate_ref) + list(labeled_select_ref)):
        if r["cloud_name"] not in total_cloud:
            total_cloud[r["cloud_name"]] = []
            order.append(r["cloud_name"])
        total_cloud[r["cloud_name"]].append((r["sp_idx"], i))
    L = _lib.lib()
    # every cloud's centres and directed chamfer means by the batched graph call: one concatenated point array, CSR offsets shifted per cloud
    xyzs, offs, ptss, sel, rows, counts = [], [np.zeros(1, np.int32)], [], [], [], []
    pbase = sbase = 0
    for name in order:
        xyz, off, pts = clouds[name]
        off = np.ascontiguousarray(off, np.int32)
        xyzs.append(np.ascontiguousarray(xyz, np.float32)); ptss.append(np.ascontiguousarray(pts, np.int32) + pbase); offs.append(off[1:] + offs[-1][-1])
        sel += [s + sbase for s, _ in total_cloud[name]]; rows += [i for _, i in total_cloud[name]]; counts.append(len(total_cloud[name]))
        pbase += len(xyz); sbase += len(off) - 1
    counts = np.asarray(counts, np.int64)
    coff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32); boff = np.concatenate([[0], np.cumsum(counts * counts)]).astype(np.int64)
    d_x = DevArray.from_host(np.concatenate(xyzs)); d_o = DevArray.from_host(np.concatenate(offs).astype(np.int32)); d_p = DevArray.from_host(np.concatenate(ptss))
    d_s = DevArray.from_host(np.asarray(sel, np.int32)); d_r = DevArray.from_host(np.asarray(rows, np.int32))
    d_coff = DevArray.from_host(coff); d_boff = DevArray.from_host(boff)
    d_c = DevArray((N, 3), np.float64); d_dir = DevArray((int(boff[-1]),), np.float64); d_a = DevArray((int(boff[-1]),), np.float64)
    _lib.check(L.ssdr_cloud_graph_batch_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, d_coff.ptr, d_boff.ptr, len(order), N, int(counts.max()), 0, d_c.ptr, d_dir.ptr, d_a.ptr, None))
    d_f = DevArray.from_host(f); d_v = DevArray((N, F), np.float32); d_adj = DevArray((N, N), np.float32)
    _lib.check(L.ssdr_create_adj_dev(d_f.ptr, N, F, d_c.ptr, d_dir.ptr, d_coff.ptr, d_boff.ptr, len(order), int(counts.max()), d_r.ptr, d_v.ptr, d_adj.ptr, None))
    _lib.sync()
    return d_v.to_host(), d_adj.to_host()


class kCenterGreedy:
    """kcenterGreedy.py:46-128 (the part the AL loop calls: select_batch_ with a non-empty already_selected)."""

    def __init__(self, X, metric="euclidean"):
        assert metric == "euclidean"
        self.features = np.ascontiguousarray(X, np.float64).reshape(len(X), -1)

    def select_batch_(self, already_selected, N, **kwargs):
        a = np.ascontiguousarray(already_selected, np.int32)
        d_f = DevArray.from_host(self.features); d_a = DevArray.from_host(a); d_o = DevArray((N,), np.int32)
        _lib.check(_lib.lib().ssdr_kcenter_dev(d_f.ptr, self.features.shape[0], self.features.shape[1], d_a.ptr, len(a), N, d_o.ptr, None))
        _lib.check(_lib.lib().ssdr_select_status(None, None))
        _lib.sync()
        return list(d_o.to_host())


def GCN_FPS_sampling(labeled_select_features, labeled_select_ref, unlabeled_candidate_features, unlabeled_candidate_ref,
                     clouds, sampling_batch, gcn_number, gcn_top, start):
    """fps_gcn_cpu.py:150-178 with the on-disk inputs replaced by `clouds`:
    {cloud_name: (xyz [n,3] f32, offsets, points)}.  refs are lists of {"cloud_name", "sp_idx"} as in the reference.
    Returns {cloud_name: [sp_idx, ...]} in selection order."""
    n_unl, n_lab = len(unlabeled_candidate_ref), len(labeled_select_ref)
    N, D = n_unl + n_lab, np.asarray(unlabeled_candidate_features).shape[1]
    if int(gcn_top) > N:       # the reference's mask[source_idx, arg_idx] = 1.0 cannot broadcast (N, gcn_top) against (N, N) (:155-159)
        raise IndexError("shape mismatch: indexing arrays could not be broadcast together with shapes (%d,%d) (%d,%d)" % (N, int(gcn_top), N, N))
    V = np.concatenate([np.asarray(unlabeled_candidate_features, np.float64).reshape(n_unl, D),
                        np.asarray(labeled_select_features, np.float64).reshape(n_lab, D)])
    total_cloud, order = {}, []                 # fps_adj_all :47-62
    for i, r in enumerate(list(unlabeled_candidate_ref) + list(labeled_select_ref)):
        if r["cloud_name"] not in total_cloud:
            total_cloud[r["cloud_name"]] = []
            order.append(r["cloud_name"])
        total_cloud[r["cloud_name"]].append((r["sp_idx"], i))
    d_v = DevArray.from_host(V); d_comb = DevArray.from_host(V)
    d_tmp = [DevArray((N, D), np.float64), DevArray((N, D), np.float64)]
    blocks = []
    L = _lib.lib()
    for name in order:
        xyz, off, pts = clouds[name]
        off = np.ascontiguousarray(off, np.int32)
        sel = np.array([s for s, _ in total_cloud[name]], np.int32)
        rows = np.array([i for _, i in total_cloud[name]], np.int32)
        n = len(sel)
        d = dict(x=DevArray.from_host(np.ascontiguousarray(xyz, np.float32)), o=DevArray.from_host(off),
                 p=DevArray.from_host(np.ascontiguousarray(pts, np.int32)), s=DevArray.from_host(sel), r=DevArray.from_host(rows),
                 c=DevArray((n, 3), np.float64), d=DevArray((n, n), np.float64), a=DevArray((n, n), np.float64), n=n)
        _lib.check(L.ssdr_cloud_graph_dev(d["x"].ptr, d["o"].ptr, d["p"].ptr, d["s"].ptr, n, int((off[sel + 1] - off[sel]).max()), int(gcn_top),
                                          d["c"].ptr, d["d"].ptr, d["a"].ptr, None))
        blocks.append(d)
    src = d_v
    for hop in range(int(gcn_number)):          # :162-167
        dst = d_tmp[hop & 1]
        for d in blocks:
            _lib.check(L.ssdr_propagate_dev(d["a"].ptr, d["n"], d["r"].ptr, src.ptr, D, dst.ptr, d_comb.ptr, None))
        src = dst
    d_out = DevArray((sampling_batch,), np.int32)
    _lib.check(L.ssdr_fps_dev(d_comb.ptr, n_unl, D, int(start), sampling_batch, d_out.ptr, None))   # FPS over comb[:n_unl] (:169-170)
    _lib.check(L.ssdr_select_status(None, None))
    _lib.sync()
    file_list = {}
    for i in d_out.to_host():
        r = unlabeled_candidate_ref[int(i)]
        file_list.setdefault(r["cloud_name"], []).append(r["sp_idx"])
    return file_list


# ---- the trained-GCN selector: gcn.GCN_sampling (gcn.py:193-263), csrc/select_gcn.hip -------------------------------------------------------
GCN_NPARAM, GCN_FUSED_CAP = 4353, 1024
GCN_FORMS = {"auto": 0, "general": 1, "fused": 2}
GCN_ST_SINGLETON, GCN_ST_NO_LABELLED, GCN_ST_SUBSTITUTED, GCN_ST_OVERSIZE = 32, 64, 128, 256


def gcn_init_params(seed):
    """The initial W1 [32,128], b1 [128], W3 [128], b3 [1] as one float32 array, drawn as GraphConvolution.reset_parameters does (gcn.py:32-36):
    uniform +-1/sqrt(out_features), i.e. +-1/sqrt(128) for gc1 and +-1 for gc3 — from NumPy's generator seeded with `seed` (the reference draws from
    torch's global one)."""
    rng = np.random.RandomState(int(seed) & 0xffffffff)
    s = 1.0 / np.sqrt(128.0)
    return np.concatenate([rng.uniform(-s, s, 32 * 128), rng.uniform(-s, s, 128), rng.uniform(-1.0, 1.0, 128), rng.uniform(-1.0, 1.0, 1)]).astype(np.float32)


def gcn_status_check(info, cloud_names=None):
    """ValueError for what the reference would train on NaN for: a cloud with a single row (zero column sum), no labelled row (empty mean)."""
    st = int(info[0])
    if st & GCN_ST_SINGLETON:
        c = int(info[1])
        name = cloud_names[c] if cloud_names is not None and 0 <= c < len(cloud_names) else c
        raise ValueError("GCN_sampling: cloud %r contributes a single row to the graph: its adjacency column sums to 0 (the reference divides by it, "
                         "gcn.py:185-187)" % (name,))
    if st & GCN_ST_NO_LABELLED:
        raise ValueError("GCN_sampling: no labelled row: the loss is a mean over an empty set (gcn.py:81-83)")
    if st & GCN_ST_OVERSIZE:
        raise ValueError("GCN_sampling: a cloud's block exceeds the fused form's %d rows (n_max understated)" % GCN_FUSED_CAP)


class GcnGraph:
    """The block adjacency of the trained-GCN branch on the device, and the calls that run over it.  rows[g] = the row (in the reference's
    [unlabelled | labelled] order) of grouped position g; counts = rows per cloud.  cap_rows > the live row count leaves spare (never read) rows."""

    def __init__(self, counts, rows, n_unl, cap_rows=None, cloud_names=None):
        counts = np.asarray(counts, np.int64)
        self.counts, self.rows_h = counts, np.asarray(rows, np.int32)
        self.N = int(counts.sum()); self.n_unl = int(n_unl); self.n_lab = self.N - self.n_unl
        self.cap = int(cap_rows or self.N); self.B = len(counts); self.n_max = int(counts.max())
        self.cloud_names = cloud_names
        self.coff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32); self.boff = np.concatenate([[0], np.cumsum(counts * counts)]).astype(np.int64)
        self.d_coff, self.d_boff = DevArray.from_host(self.coff), DevArray.from_host(self.boff)
        self.d_rows = DevArray.from_host(np.concatenate([self.rows_h, np.zeros(self.cap - self.N, np.int32)]))
        self.d_counts = DevArray.from_host(np.array([self.n_unl, self.n_lab, self.N, self.n_max, 0, 0, 0, 0], np.int32))
        self.d_v = DevArray((self.cap, 32), np.float32); self.d_adj = DevArray((int(self.boff[-1]),), np.float32); self.d_adjT = DevArray((int(self.boff[-1]),), np.float32)
        self.d_rowcloud = DevArray((self.cap,), np.int32); self.d_info = DevArray((8,), np.int32)

    @classmethod
    def from_clouds(cls, featuresV, labeled_select_ref, unlabeled_candidate_ref, clouds, cap_rows=None):
        """create_adj's inputs (see create_adj above) -> the blocks, by ssdr_cloud_graph_batch_dev + ssdr_gcn_block_adj_dev"""
        f = np.ascontiguousarray(featuresV, np.float32)
        N = len(f)
        total_cloud, order = {}, []
        for i, r in enumerate(list(unlabeled_candidate_ref) + list(labeled_select_ref)):
            if r["cloud_name"] not in total_cloud:
                total_cloud[r["cloud_name"]] = []
                order.append(r["cloud_name"])
            total_cloud[r["cloud_name"]].append((r["sp_idx"], i))
        xyzs, offs, ptss, sel, rows, counts = [], [np.zeros(1, np.int32)], [], [], [], []
        pbase = sbase = 0
        for name in order:
            xyz, off, pts = clouds[name]
            off = np.ascontiguousarray(off, np.int32)
            xyzs.append(np.ascontiguousarray(xyz, np.float32)); ptss.append(np.ascontiguousarray(pts, np.int32) + pbase); offs.append(off[1:] + offs[-1][-1])
            sel += [s + sbase for s, _ in total_cloud[name]]; rows += [i for _, i in total_cloud[name]]; counts.append(len(total_cloud[name]))
            pbase += len(xyz); sbase += len(off) - 1
        G = cls(counts, rows, len(unlabeled_candidate_ref), cap_rows, order)
        L = _lib.lib()
        d_x = DevArray.from_host(np.concatenate(xyzs)); d_o = DevArray.from_host(np.concatenate(offs).astype(np.int32)); d_p = DevArray.from_host(np.concatenate(ptss))
        d_s = DevArray.from_host(np.asarray(sel, np.int32))
        nsq = int(G.boff[-1])
        d_c = DevArray((N, 3), np.float64); d_dir = DevArray((nsq,), np.float64); d_a = DevArray((nsq,), np.float64)
        _lib.check(L.ssdr_cloud_graph_batch_dev(d_x.ptr, d_o.ptr, d_p.ptr, d_s.ptr, G.d_coff.ptr, G.d_boff.ptr, G.B, N, G.n_max, 0, d_c.ptr, d_dir.ptr, d_a.ptr, None))
        pad = np.full((G.cap - N, 32), np.nan, np.float32)
        d_f = DevArray.from_host(np.concatenate([f, pad]))
        _lib.check(L.ssdr_gcn_block_adj_dev(d_f.ptr, G.cap, 32, d_c.ptr, d_dir.ptr, G.d_coff.ptr, G.d_boff.ptr, G.B, G.n_max, G.d_rows.ptr, G.d_counts.ptr,
                                            G.d_v.ptr, G.d_adj.ptr, G.d_adjT.ptr, G.d_rowcloud.ptr, G.d_info.ptr, None))
        _lib.sync()
        return G

    @classmethod
    def from_blocks(cls, V, blocks, rows, n_unl, cap_rows=None):
        """a graph given outright: V [N,32] (rows in the [unlabelled | labelled] order, taken as they are) and every cloud's adjacency block"""
        G = cls([len(b) for b in blocks], rows, n_unl, cap_rows)
        V = np.ascontiguousarray(V, np.float32)
        _lib.check(_lib.lib().ssdr_memcpy_h2d(G.d_v.ptr, _lib.ptr(np.concatenate([V, np.full((G.cap - G.N, 32), np.nan, np.float32)])), G.cap * 32 * 4))
        a = np.concatenate([np.ascontiguousarray(b, np.float32).reshape(-1) for b in blocks]); t = np.concatenate([np.ascontiguousarray(np.asarray(b, np.float32).T).reshape(-1) for b in blocks])
        _lib.check(_lib.lib().ssdr_memcpy_h2d(G.d_adj.ptr, _lib.ptr(a), a.nbytes)); _lib.check(_lib.lib().ssdr_memcpy_h2d(G.d_adjT.ptr, _lib.ptr(t), t.nbytes))
        rc = np.concatenate([np.repeat(np.arange(G.B, dtype=np.int32), G.counts), np.zeros(G.cap - G.N, np.int32)])
        _lib.check(_lib.lib().ssdr_memcpy_h2d(G.d_rowcloud.ptr, _lib.ptr(rc), rc.nbytes))
        info = np.array([0, 0x7fffffff, 0, 0, 0, 0, 0, 0], np.int32)
        if (G.counts == 1).any():
            info[0], info[1] = GCN_ST_SINGLETON, int(np.flatnonzero(G.counts == 1)[0])
        _lib.check(_lib.lib().ssdr_memcpy_h2d(G.d_info.ptr, _lib.ptr(info), info.nbytes))
        return G

    def info(self):
        _lib.sync()
        return self.d_info.to_host()

    def normalised(self):
        return self.d_v.to_host()[: self.N]

    def blocks(self, transposed=False):
        a = (self.d_adjT if transposed else self.d_adj).to_host()
        return [a[self.boff[c]: self.boff[c + 1]].reshape(int(self.counts[c]), int(self.counts[c])) for c in range(self.B)]

    def _graph_args(self):
        return (self.d_v.ptr, self.d_adj.ptr, self.d_adjT.ptr, self.d_coff.ptr, self.d_boff.ptr, self.B, self.n_max, self.d_rows.ptr, self.d_rowcloud.ptr,
                self.d_counts.ptr, self.cap)

    def train(self, init, steps, p=0.3, lr=1e-3, weight_decay=5e-4, lamda=1.2, seed=0, form="auto", check=True):
        """-> (trained parameters [4353] float32, (loss at step 0, loss after the last step), info)"""
        d_p = DevArray.from_host(np.ascontiguousarray(init, np.float32).reshape(GCN_NPARAM)); d_loss = DevArray((2,), np.float32)
        _lib.check(_lib.lib().ssdr_gcn_train_dev(*self._graph_args(), d_p.ptr, d_p.ptr, int(steps), float(p), float(lr), float(weight_decay), float(lamda),
                                                 int(seed) & 0xffffffffffffffff, GCN_FORMS[form], d_loss.ptr, self.d_info.ptr, None))
        info = self.info()
        if check:
            gcn_status_check(info, self.cloud_names)
        return d_p.to_host(), d_loss.to_host(), info

    def evaluate(self, params, check=True):
        """-> (rows [N,129] float64 in the [unlabelled | labelled] order, info)"""
        d_p = DevArray.from_host(np.ascontiguousarray(params, np.float32).reshape(GCN_NPARAM))
        d_out = DevArray.from_host(np.full((self.cap, 129), -7.0))
        _lib.check(_lib.lib().ssdr_gcn_eval_dev(*self._graph_args(), d_p.ptr, d_out.ptr, self.d_info.ptr, None))
        info = self.info()
        if check:
            gcn_status_check(info, self.cloud_names)
        return d_out.to_host(), info


def GCN_sampling(labeled_select_features, labeled_select_ref, unlabeled_candidate_features, unlabeled_candidate_ref, clouds, sampling_batch, gcn_gpu=None,
                 coreGCN=True, steps=20000, dropout=0.3, seed=0, form="auto"):
    """gcn.GCN_sampling (gcn.py:193-263) with the two on-disk paths replaced by `clouds` {cloud_name: (xyz [n,3] f32, offsets, points)}: create_adj as
    blocks, `steps` Adam steps of the two-layer GCN from gcn_init_params(seed), the evaluation rows, kCenterGreedy seeded with the labelled rows.
    gcn_gpu is accepted and ignored.  Returns {cloud_name: [sp_idx, ...]} in selection order."""
    if not coreGCN:
        raise NotImplementedError("GCN_sampling: coreGCN=False (uncertainGCN, gcn.py:251-255) has no call site in the reference and is not offered")
    n_unl, n_lab = len(unlabeled_candidate_ref), len(labeled_select_ref)
    fu = np.asarray(unlabeled_candidate_features, np.float32).reshape(n_unl, 32); fl = np.asarray(labeled_select_features, np.float32).reshape(n_lab, 32)
    if n_lab == 0:
        raise ValueError("GCN_sampling: no labelled row: the loss is a mean over an empty set (gcn.py:81-83)")
    G = GcnGraph.from_clouds(np.concatenate([fu, fl]), labeled_select_ref, unlabeled_candidate_ref, clouds)
    gcn_status_check(G.info(), G.cloud_names)
    params, _, _ = G.train(gcn_init_params(seed), steps, p=dropout, seed=seed, form=form)
    feat, _ = G.evaluate(params)
    picks = kCenterGreedy(feat[: G.N]).select_batch_(np.arange(n_unl, n_unl + n_lab), int(sampling_batch))
    file_list = {}
    for i in picks:
        r = unlabeled_candidate_ref[int(i)]
        file_list.setdefault(r["cloud_name"], []).append(r["sp_idx"])
    return file_list
