"""Trainer.train_round(eval_from=): the epoch from which the voting evaluation runs, int(epochs * eval_from): 0.4 as the S3DIS train loop
(the default), 0.6 as Semantic3D's train2 (the reference's SSRD_AL_semantic3d/RandLANet.py:310)."""
import pytest

import _train_cases as TC


class _NoBatches:
    """a feeder whose epochs hold no batch: train_round's epoch arithmetic alone"""
    steps_per_epoch = 0

    def epoch_batches(self, stream):
        return iter(())


class _Tester:
    def __init__(self, net, asked, trainer):
        self.net, self.asked, self.trainer = net, asked, trainer

    def evaluate(self):
        # the learning rate has decayed once per finished epoch: the epoch is the number of decays
        self.asked.append(self.trainer.epochs_done)
        return 0.5, 0.25


@pytest.mark.parametrize("eval_from, first", [(None, 2), (0.6, 3)])
def test_first_evaluation_epoch(backend, eval_from, first):
    from ssdr_al import randlanet
    from ssdr_al.helper_tool import ConfigS3DIS
    from ssdr_al.trainer import Trainer

    class Small(ConfigS3DIS):
        num_points = 512
        num_layers = 2
        sub_sampling_ratio = [4, 4]
        d_out = [16, 64]
    W = TC.weights_for(Small, 6)
    tr = Trainer(Small).load(W)
    tr.epochs_done = 0
    decay = tr.decay
    tr.decay = lambda epoch: (decay(epoch), setattr(tr, "epochs_done", epoch))[0]
    asked = []
    tester = _Tester(randlanet.Network(Small).load(W), asked, tr)
    kw = {} if eval_from is None else dict(eval_from=eval_from)
    assert int(5 * 0.4) == 2 and int(5 * 0.6) == 3
    assert tr.train_round(_NoBatches(), 5, tester, **kw) == (0.5, 0.25)
    assert asked == list(range(first, 6)), asked
