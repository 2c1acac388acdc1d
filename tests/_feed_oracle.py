"""NumPy restatement of the reference's training-time generators, for tests/test_train_feeder.py.

Chain:       Semantic3D_Dataset_Train.get_batch (SSRD_AL_semantic3d/semantic3d_dataset_train.py:151-210), as a generalisation of _vote_oracle.Generator
             (the test datasets' get_batch): x / y centring, the class-weighted update, local rows, the activation / pseudo-label channels.
Independent: S3DIS_Dataset.spatially_regular_gen in training mode (SSDR_AL_s3dis/s3dis_dataset.py:115-154).
Augment:     tf_augment_input (semantic3d_dataset_train.py:237-276), element by element and as the reference writes it (np.matmul).
Where the reference draws from np.random the caller hands the draws in, as in _vote_oracle."""
import numpy as np

import _vote_oracle as VO


def _query(points, pick, N, perm):
    """the num_points nearest rows as this project orders the tree query (float32 key, ties by row), through the caller's shuffle"""
    n = len(points)
    d = points - pick
    key = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    order = np.argsort(key, kind="stable")[: min(N, n)]
    return order[perm] if n >= N else order[perm[perm < n]]


def _pad_rows(n, N, dup):
    """DP.data_aug (helper_tool.py:186-199) with the caller's draws: rows 0 .. n-1, then duplicates of the shuffled list"""
    take = np.minimum((np.asarray(dup, np.float32)[n:] * np.float32(n)).astype(np.int64), n - 1)
    return np.concatenate([np.arange(n), take])


class ChainGenerator(VO.Generator):
    def __init__(self, clouds, possibility, num_points, color_scale=np.float32(1.0), xy_only=False, global_rows=True, class_weight=None,
                 activation=None, pseudo=None):
        super().__init__(clouds, possibility, num_points, color_scale)
        self.xy_only, self.global_rows, self.cw, self.act, self.pse = xy_only, global_rows, class_weight, activation, pseudo

    def tile(self, noise, perm, dup):
        N = self.N
        cloud_idx = int(np.argmin(np.asarray(self.min_possibility)))                                 # :161
        point_ind = int(np.argmin(self.possibility[cloud_idx]))                                      # :164
        cl = self.clouds[cloud_idx]
        points = cl["xyz"]
        n = len(points)
        pick = points[point_ind].reshape(1, -1) + np.asarray(noise, np.float32).reshape(1, -1)       # :170-174
        queried = _query(points, pick, N, perm)                                                      # :175-178
        xyz = points[queried].copy()                                                                 # :181
        if self.xy_only:
            xyz[:, 0:2] = xyz[:, 0:2] - pick[:, 0:2]                                                 # :182
        else:
            xyz = xyz - pick
        dists = np.sum(np.square((points[queried] - pick).astype(np.float32)), axis=1)               # :196
        delta = np.square(1 - dists / np.max(dists))                                                 # :197
        if self.cw is not None:
            delta = delta * np.array([self.cw[l] for l in cl["labels"][queried]])                    # :193, :197 (IndexError past the weights)
        self.possibility[cloud_idx][queried] += delta                                                # :198
        self.min_possibility[cloud_idx] = float(np.min(self.possibility[cloud_idx]))                 # :199
        if n < N:
            rows = _pad_rows(n, N, dup)
            queried, xyz = queried[rows], xyz[rows]
        rgb = cl["rgb"].astype(np.float32)[queried] * self.scale
        o = self.off[cloud_idx]
        out = dict(cloud=cloud_idx, center=pick[0].astype(np.float32), idx=((o if self.global_rows else 0) + queried).astype(np.int32),
                   xyz=xyz.astype(np.float32), feat=np.concatenate([xyz, rgb], 1).astype(np.float32), labels=cl["labels"][queried].astype(np.int32))
        if self.act is not None:
            out["act"] = self.act[cloud_idx][queried].astype(np.float32)
        if self.pse is not None:
            out["pse"] = self.pse[cloud_idx][queried].astype(np.float32)
        return out

    def batch(self, draws):
        B = len(draws["noise"])
        tiles = [self.tile(draws["noise"][t], draws["perm"][t], draws["dup"][t]) for t in range(B)]
        out = {k: np.stack([t[k] for t in tiles]) for k in tiles[0] if k != "cloud"}
        out["cloud"] = np.array([t["cloud"] for t in tiles], np.int32)
        return out


def indep_tile(cl, act, pse, point, noise, perm, dup, N, scale=np.float32(1.0)):
    """spatially_regular_gen (s3dis_dataset.py:115-154), mode "training", with the caller's point_ind, noise, shuffle and padding draws"""
    points = cl["xyz"]
    n = len(points)
    pick = points[int(point)].reshape(1, -1) + np.asarray(noise, np.float32).reshape(1, -1)          # :122-126
    queried = _query(points, pick, N, perm)                                                          # :129-137
    xyz = points[queried] - pick                                                                     # :139-140
    if n < N:                                                                                        # :147-150
        rows = _pad_rows(n, N, dup)
        queried, xyz = queried[rows], xyz[rows]
    rgb = cl["rgb"].astype(np.float32)[queried] * scale
    return dict(center=pick[0].astype(np.float32), idx=queried.astype(np.int32), xyz=xyz.astype(np.float32),
                feat=np.concatenate([xyz, rgb], 1).astype(np.float32), labels=cl["labels"][queried].astype(np.int32),
                act=act[queried].astype(np.float32), pse=pse[queried].astype(np.float32))


def indep_batch(clouds, acts, pses, tile_cloud, tile_point, draws, N, scale=np.float32(1.0)):
    tiles = [indep_tile(clouds[c], acts[c], pses[c], p, draws["noise"][t], draws["perm"][t], draws["dup"][t], N, scale)
             for t, (c, p) in enumerate(zip(tile_cloud, tile_point))]
    return {k: np.stack([t[k] for t in tiles]) for k in tiles[0]}


def augment(xyz, rot, scale, noise=None):
    """float32(((x . R) * s) + noise) in float64, element by element: (x . R)_j = (x R0j + y R1j) + z R2j, R = [[c, -s, 0], [s, c, 0], [0, 0, 1]].
    xyz f32 [T,N,3], rot f64 [T,2] = (c, s), scale f64 [T,3], noise f64 [T,N,3] or None."""
    x, y, z = (xyz[..., k].astype(np.float64) for k in range(3))
    c, s = rot[:, 0][:, None], rot[:, 1][:, None]
    r = np.stack([(x * c + y * s) + z * 0.0, (x * (-s) + y * c) + z * 0.0, (x * 0.0 + y * 0.0) + z * 1.0], axis=-1)
    r = r * scale[:, None, :]
    if noise is not None:
        r = r + noise
    return r.astype(np.float32)


def augment_reference(xyz, rot, scale, noise):
    """tf_augment_input's own expression for one tile (:242-273), the draws handed in: returns the float64 result"""
    c, s = np.array([rot[0]]), np.array([rot[1]])
    cs0, cs1 = np.zeros_like(c), np.ones_like(c)
    R = np.stack([c, -s, cs0, s, c, cs0, cs0, cs0, cs1], axis=1)
    stacked_rots = np.reshape(R, (3, 3))
    transformed_xyz = np.reshape(np.matmul(xyz, stacked_rots), [-1, 3])
    stacked_scales = np.tile(np.asarray(scale).reshape(1, 3), [np.shape(transformed_xyz)[0], 1])
    transformed_xyz = transformed_xyz * stacked_scales
    return transformed_xyz + noise
