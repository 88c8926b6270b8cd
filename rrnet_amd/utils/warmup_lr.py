"""utils/warmup_lr.py of the reference: a multi-step schedule with a warm-up in front.

    lr(t) = base_lr * w(t) * gamma ** #{m in milestones : m <= t}
    w(t)  = 1                                                         for t >= warmup_iters
          = warmup_factor                                             "constant", t < warmup_iters
          = warmup_factor * (1 - t / warmup_iters) + t / warmup_iters "linear",   t < warmup_iters

t is the scheduler's `last_epoch` (0 after construction, +1 per step()).  The rate is a closed function of t, so
state_dict() / load_state_dict() resume it from `last_epoch` alone."""
import bisect

from torch.optim.lr_scheduler import LRScheduler


class WarmupMultiStepLR(LRScheduler):
    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=1250, warmup_method="linear",
                 last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        if warmup_method not in ("constant", "linear"):
            raise ValueError("Only 'constant' or 'linear' warmup_method accepted, got {}".format(warmup_method))
        self.milestones = milestones
        self.gamma = gamma
        self.warmup_factor = warmup_factor
        self.warmup_iters = warmup_iters
        self.warmup_method = warmup_method
        super().__init__(optimizer, last_epoch)

    def warmup_weight(self, t):
        if t >= self.warmup_iters:
            return 1
        if self.warmup_method == "constant":
            return self.warmup_factor
        ramp = float(t) / self.warmup_iters
        return self.warmup_factor * (1 - ramp) + ramp

    def get_lr(self):
        t = self.last_epoch
        drops = bisect.bisect_right(self.milestones, t)
        return [base * self.warmup_weight(t) * self.gamma ** drops for base in self.base_lrs]
