"""GPU: the released PEBAL recipe -- backbone and pixel decoder frozen, the whole transformer decoder trained -- through the command line with
``--differentiable_decoder``, at the tiny sizes of tests/test_train_net_gpu.py; and FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES the same way.

Unvisited ``level_embed`` rows: the tiny model (as the released 1-layer one) has one memory level and visits it, so every row of every predictor
parameter receives a gradient and "moved" needs no help from weight decay here (tests/test_decoder_backward_gpu.py covers the exactly-zero
gradient rows of a three-level one-layer decoder)."""
import math
import os

import pytest
import torch

from tests import _solver_cases as C
from tests.test_train_net_gpu import H, W, TINY_OPTS, _write_trees

pytestmark = pytest.mark.gpu


def _argv(tmp_path, out):
    C.recipe_cfg(tmp_path, C.RECIPES["pebal"][0])                                      # writes the recipe and its _BASE_ chain
    config = str(tmp_path / "a" / "b" / os.path.basename(C.RECIPES["pebal"][0]))
    return ["--config-file", config, "--cityscapes_root", str(tmp_path / "cityscapes"), "--coco_root", str(tmp_path / "coco"), "--output_dir", out,
            "--num_workers", "2", "--log_period", "1", "--differentiable_decoder"]


def _seeded_weights(tmp_path):
    """MODEL.WEIGHTS = tiny1's seeded weights as a checkpoint file.  The model's own initial weights will not do here: its in_proj weights start
    at zero, where q = k = 0 and the gradients of the q / k projections and of `query_embed` (which enters through them alone) vanish identically."""
    from rba_amd import arch as A
    path = str(tmp_path / "seeded.pth")
    torch.save({"model": {k: torch.as_tensor(v) for k, v in A.seeded_weights(A.complete(A.ARCHS["tiny1"]), 0).items()}}, path)
    return ["MODEL.WEIGHTS", path]


def test_released_pebal_recipe_trains_the_whole_decoder(tmp_path):
    from rba_amd import evaluate_ood as E
    from rba_amd import train_net
    _write_trees(tmp_path)
    out = str(tmp_path / "out" / "model")
    seen = []
    step = train_net.Trainer.step

    def recording_step(self):
        if not seen:
            seen.append({k: v.detach().clone() for k, v in self.model.state_dict().items()})
        r = step(self)
        assert math.isfinite(float(self.last_loss)) and math.isfinite(float(self.optimizer.grad_norm)) and float(self.optimizer.grad_norm) > 0
        return r
    train_net.Trainer.step = recording_step
    try:
        t = train_net.main(_argv(tmp_path, out) + TINY_OPTS + _seeded_weights(tmp_path) + ["SOLVER.MAX_ITER", "3"])
    finally:
        train_net.Trainer.step = step
    assert t.iteration == 3 and t.optimizer.step_count == 3
    predictor = t.model.sem_seg_head.predictor
    names = {"sem_seg_head.predictor." + n for n, _ in predictor.named_parameters()}
    assert set(t.optimizer.names) == names and predictor.differentiable_decoder and predictor.deep_supervision
    after = t.model.state_dict()
    for k, v in seen[0].items():
        if k in names:
            assert not torch.equal(after[k], v), f"{k} did not move"
            assert bool(torch.isfinite(after[k]).all()), k
        else:
            assert torch.equal(after[k], v), f"{k} is frozen and moved"
    model = E.get_model(os.path.join(out, "config.yaml"), os.path.join(out, "model_final.pth"), device="cuda")
    sd = model.state_dict()
    assert all(torch.equal(sd[k], after[k]) for k in after)
    image = torch.randint(0, 256, (3, H, W), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    assert bool(torch.isfinite(model.rba_scores([{"image": image}])[0]).all())


def test_object_queries_recipe_steps_the_two_query_tensors(tmp_path):
    from rba_amd import train_net
    _write_trees(tmp_path)
    out = str(tmp_path / "out" / "queries")
    before = {}
    step = train_net.Trainer.step

    def recording_step(self):
        if not before:
            before.update({k: v.detach().clone() for k, v in self.model.state_dict().items()})
        return step(self)
    train_net.Trainer.step = recording_step
    try:
        t = train_net.main(_argv(tmp_path, out) + TINY_OPTS + _seeded_weights(tmp_path) + ["MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES", "True", "SOLVER.MAX_ITER", "3"])
    finally:
        train_net.Trainer.step = step
    moved = {"sem_seg_head.predictor.query_feat.weight", "sem_seg_head.predictor.query_embed.weight"}
    assert set(t.optimizer.names) == moved
    after = t.model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v) == (k not in moved), k
