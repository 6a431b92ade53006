"""The reference's matchers (mask2former/modeling/matcher.py) on the HIP kernels: ``HungarianMatcher`` builds each image's [Q,T] cost matrix in
one ``ops.match_cost`` call (K8) -- the point sampling of all Q predictions and all T targets at P shared points, the sigmoid-CE and dice
contractions and the class term -- and solves the assignment on the host with scipy, as the reference does.  The cost is bitwise reproducible, so
the same inputs and points give the same assignment run after run."""
import torch
import torch.nn.functional as F

from .. import ops


def _empty():
    return torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64)


class HungarianMatcher(torch.nn.Module):
    """``HungarianMatcher(cost_class, cost_mask, cost_dice, num_points)`` (matcher.py:70-156).  ``forward(outputs, targets)`` with
    outputs["pred_logits"] [B,Q,K+1], outputs["pred_masks"] [B,Q,h,w], targets[i]["labels"] [T_i], targets[i]["masks"] [T_i,H,W] -> a list of
    (int64 idx_i, int64 idx_j) on the CPU, len = min(Q, T_i).  ``point_coords`` [P,2] replaces the ``num_points`` uniform points that every image
    draws (from ``generator``).  An image without targets gets two empty tensors and no launch."""

    def __init__(self, cost_class=1.0, cost_mask=1.0, cost_dice=1.0, num_points=0):
        super().__init__()
        if cost_class == 0 and cost_mask == 0 and cost_dice == 0:
            raise ValueError("all costs cant be 0")
        self.cost_class, self.cost_mask, self.cost_dice, self.num_points = cost_class, cost_mask, cost_dice, num_points

    @torch.no_grad()
    def cost_matrix(self, pred_logits, pred_masks, target, point_coords=None, generator=None):
        """one image: pred_logits [Q,K+1], pred_masks [Q,h,w], target {"labels", "masks"} (T >= 1) -> the cost [Q,T] on the device"""
        dev = pred_masks.device
        if point_coords is None:
            point_coords = torch.rand(self.num_points, 2, device=dev, generator=generator)
        prob = F.softmax(pred_logits.float(), dim=-1).contiguous()
        return ops.match_cost(pred_masks.detach().contiguous(), target["masks"].to(device=dev, dtype=torch.float32).contiguous(),
                              point_coords.contiguous(), prob, target["labels"].to(device=dev, dtype=torch.int64).contiguous(),
                              cost_mask=self.cost_mask, cost_class=self.cost_class, cost_dice=self.cost_dice)

    @torch.no_grad()
    def forward(self, outputs, targets, point_coords=None, generator=None):
        from scipy.optimize import linear_sum_assignment
        out = []
        for b, target in enumerate(targets):
            if target["labels"].numel() == 0:
                out.append(_empty())
                continue
            cost = self.cost_matrix(outputs["pred_logits"][b], outputs["pred_masks"][b], target, point_coords, generator).cpu()
            i, j = linear_sum_assignment(cost.numpy())
            out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        return out

    def __repr__(self):
        return f"Matcher HungarianMatcher(cost_class={self.cost_class}, cost_mask={self.cost_mask}, cost_dice={self.cost_dice}, num_points={self.num_points})"


class FixedMatcher(torch.nn.Module):
    """matcher.py:192-214: query k is matched to the target whose label is k (one query per class)."""

    @torch.no_grad()
    def forward(self, outputs, targets, point_coords=None, generator=None):
        out = []
        for target in targets:
            labels = target["labels"].to(device="cpu", dtype=torch.int64)
            out.append((labels.clone(), torch.arange(labels.numel(), dtype=torch.int64)))
        return out
