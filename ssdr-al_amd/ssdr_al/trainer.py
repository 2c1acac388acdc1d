"""The training half of the reference's ``RandLANet.Network`` (SSDR_AL_s3dis/RandLANet.py:36-84 graph, loss and optimiser, :217-282 ``train``,
:486-585 ``get_loss`` and the blocks) on the device: ``Trainer.step`` runs forward (batch-norm batch statistics, dropout 0.5 after fc2), the
weighted cross entropy on the pseudo labels, the backward pass and tf.train.AdamOptimizer's update in libssdr_al.so (csrc/randla_train.hip).

Weights travel as the reference-named dict that ``randlanet.Network.load`` takes (entries ``W``, ``b``, ``bn = (gamma, beta, mean, var)``,
``transposed``), raw and unfolded.  By default the scatter-adds of the backward pass are float atomics: gradients and updated weights differ in
their low bits from run to run, forward values (logits, loss, accuracy of given weights) do not.  ``Trainer(..., deterministic=True)`` (or
``set_deterministic``) replaces them with reductions in a fixed order: the same inputs then give the same bits every run.

Data-parallel: ``Trainer(..., comm=distributed.Comm)`` (or ``set_comm``) trains one replica per process on that process's share of the batch, and the
step equals the step of ONE process over the union of all ranks' tiles: batch norm over all ranks' rows (forward and backward), the loss over the
global number of valid rows, one gradient sum over ``comm`` ("Data-parallel").  Weights are never broadcast: the replicas stay
identical only if they start identical, so every rank must ``load`` the same weights (and the same ``load_state``)."""
import ctypes as C

import numpy as np

from . import _lib, randlanet
from ._lib import DevArray
from .helper_tool import ConfigS3DIS
from .synthetic import layer_specs

KINDS = ("W", "b", "gamma", "beta", "mean", "var")
XCHG_GATHER, XCHG_SUM = 0, 1                                  # SSDR_XCHG_* (include/ssdr_al.h)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)      # ssdr_exchange_fn


def _bind(L):
    if getattr(L, "_train_bound", False):
        return L
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    L.ssdr_randla_train_create.argtypes = [i32, vp, i32, i32, i32, C.POINTER(vp)]
    L.ssdr_randla_train_destroy.argtypes = [vp]
    L.ssdr_randla_train_destroy.restype = None
    L.ssdr_randla_train_num_params.argtypes = [vp]
    L.ssdr_randla_train_param_shape.argtypes = [vp, i32] + [C.POINTER(i32)] * 4
    L.ssdr_randla_train_set_param.argtypes = [vp, i32, i32, vp]
    L.ssdr_randla_train_get_param.argtypes = [vp, i32, i32, vp]
    L.ssdr_randla_train_get_grad.argtypes = [vp, i32, vp]
    L.ssdr_randla_train_set_grad.argtypes = [vp, i32, vp]
    L.ssdr_randla_train_apply_dev.argtypes = [vp, vp]
    L.ssdr_randla_train_set_loss.argtypes = [vp, vp, vp, i32]
    L.ssdr_randla_train_set_lr.argtypes = [vp, C.c_float]
    L.ssdr_randla_train_set_step_count.argtypes = [vp, C.c_int64]
    L.ssdr_randla_train_step_count.argtypes = [vp]
    L.ssdr_randla_train_step_count.restype = C.c_int64
    L.ssdr_randla_train_workspace_bytes.argtypes = [vp]
    L.ssdr_randla_train_workspace_bytes.restype = sz
    L.ssdr_randla_train_last_ms.argtypes = [vp, vp]
    L.ssdr_randla_train_dropout_mask_dev.argtypes = [u64, u64, sz, vp, vp]
    step = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ssdr_randla_train_step_dev.argtypes = step
    L.ssdr_randla_train_grads_dev.argtypes = step
    L.ssdr_randla_train_forward_dev.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.ssdr_randla_train_export.argtypes = [vp, vp]
    L.ssdr_randla_train_status.argtypes = [vp, C.POINTER(i32)]
    L.ssdr_randla_train_set_deterministic.argtypes = [vp, i32]
    L.ssdr_randla_train_deterministic.argtypes = [vp]
    L.ssdr_randla_train_set_exchange.argtypes = [vp, EXCHANGE_FN, vp, i32, i32]
    L.ssdr_randla_train_exchange.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.ssdr_randla_train_dropout_mask_range_dev.argtypes = [u64, u64, u64, sz, vp, vp]
    L.ssdr_bn_stats_merge_dev.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.ssdr_rank_sums_merge_dev.argtypes = [vp, i32, i32, vp, vp]
    L._train_bound = True
    return L


class Trainer:
    """``Trainer(config).load(weights)``, then ``step(batch)`` per ``TrainFeeder`` batch, ``loss()`` / ``accuracy()`` when a number is wanted and
    ``export_to(network)`` for ``infer``, ``VoteTester`` or ``WholeCloudPredictor``.  ``train_round(feeder, epochs, tester)`` is ``Network.train``.

    comm: a ``distributed.Comm`` (one process per GPU).  Every rank steps on its own tiles and ends each step with the weights of one process
    stepping on all ranks' tiles, the same bits on every rank.  The replicas stay identical only if they start identical: every rank must ``load``
    the same weights.  Every rank must make the same calls in the same order (a rank that skips a step leaves the others waiting in a collective)."""

    def __init__(self, config=ConfigS3DIS, in_dim=6, class_weights=None, ignored_labels=(), lr=None, seed=0, deterministic=False, comm=None):
        self.config, self.in_dim, self.seed = config, int(in_dim), int(seed)
        self.L, self.Cn = int(config.num_layers), int(config.num_classes)
        self._h = C.c_void_p()
        self._lib = L = _bind(_lib.lib())
        _lib.check(L.ssdr_init(0))
        d = np.asarray(config.d_out[: self.L], np.int32)
        _lib.check(L.ssdr_randla_train_create(self.L, _lib.ptr(d), config.k_n, self.Cn, self.in_dim, C.byref(self._h)))
        self.specs = layer_specs(tuple(config.d_out[: self.L]), self.Cn, self.in_dim)
        # tensor index of (unit, kind), as the library enumerates them
        self.index, self.shapes = {}, {}
        for i in range(L.ssdr_randla_train_num_params(self._h)):
            u, k, r, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            _lib.check(L.ssdr_randla_train_param_shape(self._h, i, C.byref(u), C.byref(k), C.byref(r), C.byref(c)))
            self.index[(u.value, KINDS[k.value])] = i
            self.shapes[i] = (r.value, c.value) if k.value == 0 else (c.value,)
        assert max(u for u, _ in self.index) == len(self.specs) - 1, "the library's unit table and synthetic.layer_specs disagree"
        self.ignored = tuple(int(i) for i in ignored_labels)
        cw = None if class_weights is None else np.ascontiguousarray(np.asarray(class_weights, np.float32).reshape(-1))
        if cw is not None and len(cw) != self.Cn:
            raise ValueError("Trainer: %d class weights for %d classes" % (len(cw), self.Cn))
        ign = np.asarray(self.ignored, np.int32)
        _lib.check(L.ssdr_randla_train_set_loss(self._h, _lib.ptr(cw), _lib.ptr(ign) if len(ign) else None, len(ign)))
        self.lr = float(getattr(config, "learning_rate", 1e-2) if lr is None else lr)
        self.set_lr(self.lr)
        self._loss, self._acc = DevArray((1,), np.float32), DevArray((1,), np.float32)
        self._mask = None
        self._last_stream = None
        self._comm, self._hook, self._hook_error, self.exchanges = None, None, None, 0
        if deterministic:
            self.set_deterministic(True)
        if comm is not None:
            self.set_comm(comm)

    def __del__(self):
        try:
            if self._h:
                self._lib.ssdr_randla_train_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- weights and optimiser state ---------------------------------------------------------------------------------------
    def _tensors(self):
        """(scope, key, tensor index) of every tensor of the dict form, graph order"""
        for u, (name, cin, cout, bias, bn, act, transposed) in enumerate(self.specs):
            yield name, "W", self.index[(u, "W")]
            if bias:
                yield name, "b", self.index[(u, "b")]
            if bn:
                for k in ("gamma", "beta", "mean", "var"):
                    yield name, k, self.index[(u, k)]

    def _put(self, i, which, a):
        a = np.ascontiguousarray(a, np.float32)
        if a.shape != self.shapes[i]:
            raise ValueError("Trainer: tensor %d is %s, got %s" % (i, self.shapes[i], a.shape))
        _lib.check(self._lib.ssdr_randla_train_set_param(self._h, i, which, _lib.ptr(a)))

    def _get(self, i, which):
        a = np.empty(self.shapes[i], np.float32)
        _lib.check(self._lib.ssdr_randla_train_get_param(self._h, i, which, _lib.ptr(a)))
        return a

    def load(self, weights):
        """reference-named weights (randlanet.Network.load's dict); Adam's moments and the step count are left as they are"""
        for name, key, i in self._tensors():
            ent = weights[name]
            if key in ("W", "b"):
                self._put(i, 0, ent[key])
            else:
                self._put(i, 0, ent["bn"][("gamma", "beta", "mean", "var").index(key)])
        return self

    def weights(self):
        out = {}
        for u, (name, cin, cout, bias, bn, act, transposed) in enumerate(self.specs):
            ent = {"W": self._get(self.index[(u, "W")], 0), "b": None, "bn": None, "act": act, "transposed": transposed}
            if bias:
                ent["b"] = self._get(self.index[(u, "b")], 0)
            if bn:
                ent["bn"] = tuple(self._get(self.index[(u, k)], 0) for k in ("gamma", "beta", "mean", "var"))
            out[name] = ent
        return out

    def grads(self):
        """{(scope, key): gradient} of the last step() / grads_arrays() call, key in W, b, gamma, beta"""
        out = {}
        for name, key, i in self._tensors():
            if key in ("mean", "var"):
                continue
            a = np.empty(self.shapes[i], np.float32)
            _lib.check(self._lib.ssdr_randla_train_get_grad(self._h, i, _lib.ptr(a)))
            out[(name, key)] = a
        return out

    def state(self):
        """everything a snapshot needs, as plain NumPy: the weights, Adam's moments, the step count, the learning rate"""
        mom = {}
        for name, key, i in self._tensors():
            if key not in ("mean", "var"):
                mom[(name, key)] = (self._get(i, 1), self._get(i, 2))
        return {"weights": self.weights(), "adam": mom, "step": self.step_count(), "lr": self.lr}

    def load_state(self, st):
        self.load(st["weights"])
        for name, key, i in self._tensors():
            if key not in ("mean", "var"):
                m, v = st["adam"][(name, key)]
                self._put(i, 1, m)
                self._put(i, 2, v)
        _lib.check(self._lib.ssdr_randla_train_set_step_count(self._h, int(st["step"])))
        self.set_lr(st["lr"])
        return self

    def step_count(self):
        return int(self._lib.ssdr_randla_train_step_count(self._h))

    def set_lr(self, lr):
        """takes effect at the next step"""
        self.lr = float(lr)
        _lib.check(self._lib.ssdr_randla_train_set_lr(self._h, self.lr))
        return self

    def decay(self, epoch):
        """learning_rate *= config.lr_decays[epoch] (RandLANet.py:258-260)"""
        return self.set_lr(self.lr * float(self.config.lr_decays[epoch]))

    def set_deterministic(self, flag):
        """True: the backward scatters add in a fixed order (no float atomics), gradients and weights are reproducible bit for bit; takes effect
        at the next call, which plans the (larger) workspace again.  False (the default): the atomic kernels."""
        _lib.check(self._lib.ssdr_randla_train_set_deterministic(self._h, 1 if flag else 0))
        return self

    @property
    def deterministic(self):
        return bool(self._lib.ssdr_randla_train_deterministic(self._h))

    def set_comm(self, comm):
        """comm: a ``distributed.Comm``: from the next call on, ``step`` / ``grads_arrays`` / ``forward_arrays(is_training=True)`` meet the other ranks
        (class docstring); None: back to one process.  The collectives are enqueued on the call's stream by a callback of the library; an exception
        raised in it fails the call and is raised again by the call.  Every rank must hold the same weights when this is set."""
        if comm is None:
            _lib.check(self._lib.ssdr_randla_train_set_exchange(self._h, EXCHANGE_FN(), None, 0, 1))
            self._comm = self._hook = None
            return self

        def hook(user, op, send, recv, count, stream):
            try:
                if op == XCHG_GATHER:
                    comm.allgather_(comm.raw_view(send, count), comm.raw_view(recv, count * comm.world), stream)
                elif op == XCHG_SUM:
                    out = comm.raw_view(recv, count)
                    if send != recv:
                        with comm.on_stream(stream):
                            out.copy_(comm.raw_view(send, count))
                    comm.allreduce_sum_(out, stream)
                else:
                    raise ValueError("Trainer: unknown exchange op %d" % op)
                self.exchanges += 1
                return 0
            except BaseException as e:                      # nothing may unwind through the library's frames
                self._hook_error = e
                return 1
        cb = EXCHANGE_FN(hook)
        _lib.check(self._lib.ssdr_randla_train_set_exchange(self._h, cb, None, int(comm.rank), int(comm.world)))
        self._comm, self._hook = comm, cb                   # the library keeps the pointer: the trampoline lives as long as it is set
        return self

    @property
    def comm(self):
        return self._comm

    def _check(self, status):
        """_lib.check, after the exception the exchange callback stored during the call (if any)"""
        err, self._hook_error = self._hook_error, None
        if err is not None:
            raise err
        _lib.check(status)

    def workspace_bytes(self):
        return int(self._lib.ssdr_randla_train_workspace_bytes(self._h))

    def last_ms(self):
        """(forward, loss + backward, update) milliseconds of the last call, from HIP events (waits for it)"""
        out = np.zeros(3, np.float32)
        _lib.check(self._lib.ssdr_randla_train_last_ms(self._h, _lib.ptr(out)))
        return tuple(float(x) for x in out)

    # ---- steps ---------------------------------------------------------------------------------------------------------------
    def _pyramid(self, arrays):
        L = self.L
        if len(arrays) < 4 * L + 4:
            raise ValueError("Trainer: the input list has %d arrays, expected at least %d" % (len(arrays), 4 * L + 4))
        arr = C.c_void_p * L
        xyz, neigh, pool, up = (arrays[k * L:(k + 1) * L] for k in range(4))
        feat, labels, act, pse = arrays[4 * L:4 * L + 4]
        B, N = int(xyz[0].shape[0]), int(xyz[0].shape[1])
        r = np.asarray(self.config.sub_sampling_ratio[:L], np.int32)
        ptrs = [arr(*[a.ptr for a in lst]) for lst in (xyz, neigh, pool, up)]
        return B, N, r, ptrs, feat, labels, act, pse

    def make_mask(self, B, N, stream=None, step=None, first_row=None):
        """the dropout mask of (seed, step) for a [B, N] batch, on the device (u8 [B N, 32]).  first_row: the batch's first ELEMENT in the mask of
        the union of all ranks' batches; with a communicator it defaults to ``comm.rank * B * N * 32`` (every rank holds B tiles: a rank's mask is
        then its slice of the union's), without one to 0.  Ranks with uneven shares pass it, or their own ``mask=`` to the step."""
        n = B * N * 32
        if self._mask is None or self._mask.shape != (n,):
            self._mask = DevArray((n,), np.uint8)
        t = self.step_count() if step is None else int(step)
        if first_row is None:
            first_row = self._comm.rank * n if self._comm is not None else 0
        _lib.check(self._lib.ssdr_randla_train_dropout_mask_range_dev(self.seed, t, int(first_row), n, self._mask.ptr, stream))
        return self._mask

    def _call(self, fn, arrays, stream, mask):
        B, N, r, ptrs, feat, labels, act, pse = self._pyramid(arrays)
        if act.dtype != np.float32 or pse.dtype != np.float32 or labels.dtype != np.int32:
            raise ValueError("Trainer: labels are int32, activation and pseudo float32 (as TrainFeeder leaves them)")
        if mask is None:
            mask = self.make_mask(B, N, stream)
        self._keep = (arrays, mask, ptrs)            # the launches read them after this call returns
        self._last_stream = stream
        self._check(fn(self._h, B, N, feat.ptr, ptrs[0], _lib.ptr(r), ptrs[1], ptrs[2], ptrs[3], labels.ptr, act.ptr, pse.ptr, mask.ptr,
                       self._loss.ptr, self._acc.ptr, stream))

    def step_arrays(self, arrays, stream=None, mask=None):
        """One training step on device arrays in the reference's input_list order: [xyz_0.., neigh_0.., pool_0.., up_0.., features, labels,
        activation, pseudo, ...] (s3dis_dataset.py:180-181).  mask: a u8 [B N, 32] device array in place of the generated dropout mask.  Enqueue only."""
        self._call(self._lib.ssdr_randla_train_step_dev, arrays, stream, mask)
        return self

    def grads_arrays(self, arrays, stream=None, mask=None):
        """forward and backward without the update (weights, moving statistics and the step count stay): see grads()"""
        self._call(self._lib.ssdr_randla_train_grads_dev, arrays, stream, mask)
        return self

    def step(self, batch, stream=None, mask=None):
        """One step on a ``training.FeedBatch``; releases the batch on ``stream`` behind the step's launches."""
        try:
            self.step_arrays(batch.arrays, stream, mask)
        finally:
            batch.release(stream)
        return self

    def forward_arrays(self, arrays, is_training=False, stream=None, mask=None):
        """(logits [B N, C], last_second_features [B N, 32]) as device arrays.  is_training: batch statistics and dropout (the moving statistics stay)."""
        B, N, r, ptrs, feat = self._pyramid(arrays)[:5]
        if is_training and mask is None:
            mask = self.make_mask(B, N, stream)
        logits, f32 = DevArray((B * N, self.Cn), np.float32), DevArray((B * N, 32), np.float32)
        self._keep = (arrays, mask, ptrs)
        self._last_stream = stream
        self._check(self._lib.ssdr_randla_train_forward_dev(self._h, B, N, feat.ptr, ptrs[0], _lib.ptr(r), ptrs[1], ptrs[2], ptrs[3],
                                                            mask.ptr if mask is not None else None, 1 if is_training else 0, logits.ptr, f32.ptr, stream))
        return logits, f32

    def loss(self):
        """the last step's loss (waits for its stream)"""
        _lib.sync(self._last_stream)
        return float(self._loss.to_host(self._last_stream)[0])

    def accuracy(self):
        _lib.sync(self._last_stream)
        return float(self._acc.to_host(self._last_stream)[0])

    def status(self, stream=None):
        """the status bits the calls on ``stream`` raised (1: a loss without a valid row, 2: a label outside the table); clears them"""
        bits = C.c_int(0)
        self._lib.ssdr_randla_train_status(stream, C.byref(bits))
        return bits.value

    # ---- hand-over to inference --------------------------------------------------------------------------------------------
    def export_to(self, network=None):
        """folds the batch norms with the moving statistics into ``network`` (a new ``randlanet.Network`` when None) and returns it"""
        if network is None:
            network = randlanet.Network(self.config, self.in_dim)
        _lib.sync(self._last_stream)
        _lib.check(self._lib.ssdr_randla_train_export(self._h, network._h))
        return network

    def train_round(self, feeder, epochs, tester=None, eval_from=0.4):
        """``Network.train`` (RandLANet.py:217-282): per epoch the feeder's batches, then the decay; from int(eval_from * epochs) on the voting
        evaluation through ``tester`` (an ``evaluate.VoteTester``, whose network is reloaded from this trainer).  eval_from: 0.4 as S3DIS's train;
        Semantic3D's train2 starts at 0.6 (SSRD_AL_semantic3d/RandLANet.py:310).  Keeps the best state in ``best_state`` and
        returns (best_mIoU, best_OA).  Starts from config.learning_rate (reset_lr, :213-215).

        With a communicator every rank's feeder holds that rank's clouds and every rank steps once per batch, so all feeders must give the same number
        of batches per epoch: the ranks compare their counts before each epoch and EVERY rank raises when they differ (unequal counts would leave
        the longer ranks waiting in a collective for ever).  The evaluation stays replicated: each rank evaluates its own tester."""
        self.set_lr(float(getattr(self.config, "learning_rate", self.lr)))
        best_miou, best_oa, self.best_state = 0, 0, None
        for epoch in range(1, epochs + 1):
            if self._comm is not None:
                counts = self._comm.allgather_host(np.asarray([int(feeder.steps_per_epoch)], np.int64)).reshape(-1)
                if len(set(counts.tolist())) != 1:
                    raise ValueError("Trainer.train_round: the ranks' feeders give %s batches per epoch; every rank must step the same number of times"
                                     % counts.tolist())
            for batch in feeder.epoch_batches(None):
                self.step(batch)
            self.decay(epoch)
            if tester is not None and epoch >= int(epochs * eval_from):
                self.export_to(tester.net)
                m_iou, oa = tester.evaluate()
                if m_iou > best_miou:
                    best_miou, best_oa, self.best_state = m_iou, oa, self.state()
        return best_miou, best_oa
