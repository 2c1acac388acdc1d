"""NumPy restatement of the reference's test-time voting loop, for tests/test_vote_tester.py.

Generator: get_batch of S3/s3dis_dataset_test.py:97-151 (the same loop in the Semantic3D flavour, semantic3d_dataset_test3.py:129-193) with
this project's conventions where the reference draws from np.random: the caller hands in the noise, one shuffle permutation of [0, num_points)
per tile and the padding draws (tests/test_tile.py, tests/test_predict_clouds.py).  Loop: Network.evaluate_test_s3dis, S3/RandLANet.py:290-424."""
import numpy as np


def make_case(sizes, seed=7):
    """clouds and the initial map: uniform points in a 3 x 2.5 x 2 box, map = random * 1e-3 (init_possibility, test.py:85-92), colours, labels and a raw
    cloud per sub-cloud (proj_idx, raw_labels) from a second stream.  Returns (clouds, possibility, rng); rng goes on to draw the noise."""
    rng = np.random.default_rng(seed)
    xyz = [(rng.random((n, 3), dtype=np.float32) * np.array([3, 2.5, 2], np.float32)).astype(np.float32) for n in sizes]
    poss = [rng.random(n) * 1e-3 for n in sizes]
    r2 = np.random.default_rng(seed + 1000)
    clouds = []
    for p in xyz:
        n = len(p)
        clouds.append(dict(xyz=p, rgb=r2.integers(0, 256, (n, 3)).astype(np.uint8), labels=r2.integers(0, 13, n).astype(np.int32),
                           proj_idx=r2.integers(0, n, 2 * n + 7).astype(np.int32), raw_labels=r2.integers(0, 13, 2 * n + 7).astype(np.int32)))
    return clouds, poss, rng


def add_ties(poss):
    """two equal cloud minima (clouds 0 and 2), two equal minima inside cloud 0"""
    poss[0][5] = poss[0][9] = 0.0
    poss[2][17] = 0.0
    return poss


def draw_batch(rng, rng_perm, B, N, noise_init=3.5):
    """noise as the reference draws it, one tile after the other (test.py:114); shuffles and padding draws from a stream of their own"""
    noise = np.concatenate([rng.normal(scale=noise_init / 10, size=(1, 3)).astype(np.float32) for _ in range(B)])
    perm = np.stack([rng_perm.permutation(N) for _ in range(B)]).astype(np.int32)
    dup = rng_perm.random((B, N), dtype=np.float32)
    return dict(noise=noise, perm=perm, dup=dup)


class Generator:
    def __init__(self, clouds, possibility, num_points, color_scale=np.float32(1.0 / 255.0)):
        self.clouds, self.N, self.scale = clouds, int(num_points), color_scale
        self.possibility = [np.array(p, np.float64) for p in possibility]
        self.min_possibility = [float(np.min(p)) for p in self.possibility]                          # test.py:92
        self.off = np.concatenate([[0], np.cumsum([len(c["xyz"]) for c in clouds])]).astype(np.int64)

    def cloud_arg(self):
        return np.array([int(np.argmin(p)) for p in self.possibility], np.int32)

    def tile(self, noise, perm, dup):
        N = self.N
        cloud_idx = int(np.argmin(np.asarray(self.min_possibility)))                                 # :106
        point_ind = int(np.argmin(self.possibility[cloud_idx]))                                      # :108
        cl = self.clouds[cloud_idx]
        points = cl["xyz"]
        n = len(points)
        pick = points[point_ind].reshape(1, -1) + np.asarray(noise, np.float32).reshape(1, -1)       # :112-115 (float32)
        d = points - pick
        key = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]                            # the KDTree query as this project orders it: float32 key, ties by index
        order = np.argsort(key, kind="stable")[: min(N, n)]                                          # :117-122
        queried = order[perm] if n >= N else order[perm[perm < n]]                                   # :125, the caller's permutation
        xyz = points[queried] - pick                                                                 # :127-128
        dists = np.sum(np.square((points[queried] - pick).astype(np.float32)), axis=1)               # :132
        delta = np.square(1 - dists / np.max(dists))                                                 # :133
        self.possibility[cloud_idx][queried] += delta                                                # :134
        self.min_possibility[cloud_idx] = float(np.min(self.possibility[cloud_idx]))                 # :135
        if n < N:                                                                                    # :137-141, DP.data_aug with the caller's draws
            take = np.minimum((np.asarray(dup, np.float32)[n:] * np.float32(n)).astype(np.int64), n - 1)
            rows = np.concatenate([np.arange(n), take])
            queried, xyz = queried[rows], xyz[rows]
        rgb = cl["rgb"].astype(np.float32)[queried] * self.scale
        return dict(cloud=cloud_idx, center=pick[0].astype(np.float32), idx=(self.off[cloud_idx] + queried).astype(np.int32), local_idx=queried.astype(np.int32),
                    xyz=xyz.astype(np.float32), feat=np.concatenate([xyz, rgb], 1).astype(np.float32),
                    labels=None if cl.get("labels") is None else cl["labels"][queried].astype(np.int32))

    def batch(self, draws):
        B = len(draws["noise"])
        tiles = [self.tile(draws["noise"][t], draws["perm"][t], draws["dup"][t]) for t in range(B)]
        out = {k: np.stack([t[k] for t in tiles]) for k in ("center", "idx", "xyz", "feat")}
        out["cloud"] = np.array([t["cloud"] for t in tiles], np.int32)
        out["labels"] = None if tiles[0]["labels"] is None else np.stack([t["labels"] for t in tiles])
        return out


def vote(test_probs, idx, probs, test_smooth=0.95):
    """RandLANet.py:330-334 on the concatenated array with global rows: tile by tile, in batch order"""
    B, N = idx.shape
    probs = probs.reshape(B, N, -1)
    for j in range(B):
        p_idx = idx[j]
        test_probs[p_idx] = test_smooth * test_probs[p_idx] + (1 - test_smooth) * probs[j]            # :334
    return test_probs


def iou_from_confusions(confusions):            # helper_tool.py:237-262, restated (tests/test_evaluate.py)
    confusions = np.asarray(confusions)
    TP = np.diagonal(confusions, axis1=-2, axis2=-1)
    TP_plus_FN = np.sum(confusions, axis=-1)
    TP_plus_FP = np.sum(confusions, axis=-2)
    IoU = TP / (TP_plus_FP + TP_plus_FN - TP + 1e-6)
    mask = TP_plus_FN < 1e-3
    counts = np.sum(1 - mask, axis=-1, keepdims=True)
    mIoU = np.sum(IoU, axis=-1, keepdims=True) / (counts + 1e-6)
    IoU += mask * mIoU
    return IoU


def final_metrics(clouds, test_probs, off, num_classes):
    """RandLANet.py:353-419 from the voted probabilities: (sub confusion, rescaled sub IoUs, full confusion, full IoUs, m_IoU, OA)"""
    from sklearn.metrics import confusion_matrix
    lv = np.arange(num_classes)
    val_proportions = np.zeros(num_classes, np.float32)                                              # :298-303
    for i in lv:
        val_proportions[i] = np.sum([np.sum(c["raw_labels"] == i) for c in clouds])
    sub, full, correct, seen = [], [], 0, 0
    for c, cl in enumerate(clouds):
        probs = test_probs[off[c]:off[c + 1]]
        sub.append(confusion_matrix(cl["labels"], np.argmax(probs, axis=1).astype(np.int32), labels=lv))          # :353-359
        preds = np.argmax(probs[cl["proj_idx"], :], axis=1).astype(np.uint8)                                        # :381-394
        correct += np.sum(preds == cl["raw_labels"]); seen += len(cl["raw_labels"])
        full.append(confusion_matrix(cl["raw_labels"], preds, labels=lv))
    sub_conf = np.sum(np.stack(sub), axis=0)
    Cm = sub_conf.astype(np.float32)                                                                 # :362
    Cm *= np.expand_dims(val_proportions / (np.sum(Cm, axis=1) + 1e-6), 1)                           # :365
    sub_ious = iou_from_confusions(Cm)
    conf = np.sum(np.stack(full), axis=0)                                                            # :406
    ious = iou_from_confusions(conf)
    return dict(sub_confusion=sub_conf, sub_ious=sub_ious, confusion=conf, ious=ious, m_iou=float(np.mean(ious)), oa=correct / float(seen))
