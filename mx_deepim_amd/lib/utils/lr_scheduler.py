"""Learning-rate schedule of the training loop: WarmupMultiFactorScheduler (lib/utils/lr_scheduler.py:11-66 over
mx.lr_scheduler.LRScheduler) and the arithmetic train.py:244-254 feeds it with."""
import logging

logger = logging.getLogger(__name__)


class WarmupMultiFactorScheduler(object):
    """lr(num_update) = base_lr · factor^(number of entries of `step` that num_update has passed), or warmup_lr while
    warmup and num_update < warmup_step. Stateful as the reference is: base_lr is multiplied when a boundary is crossed (with the
    "Update[%d]: Change learning rate to %0.5e" line), in a while loop so that one call can cross several."""

    def __init__(self, step, factor=1, warmup=False, warmup_lr=0, warmup_step=0, base_lr=0.01, logger=None):
        assert isinstance(step, list) and len(step) >= 1
        for i, _step in enumerate(step):
            if i != 0 and step[i] <= step[i - 1]:
                raise ValueError("Schedule step must be an increasing integer list")
            if _step < 1:
                raise ValueError("Schedule step must be greater or equal than 1 round")
        if factor > 1.0:
            raise ValueError("Factor must be no more than 1 to make lr reduce")
        self.base_lr = base_lr      # mx.lr_scheduler.LRScheduler's default 0.01; the optimizer sets it to its learning_rate
        self.step = step
        self.cur_step_ind = 0
        self.factor = factor
        self.count = 0
        self.warmup = warmup
        self.warmup_lr = warmup_lr
        self.warmup_step = warmup_step
        self.logger = logger

    def __call__(self, num_update):
        if self.warmup and num_update < self.warmup_step:
            return self.warmup_lr
        while self.cur_step_ind <= len(self.step) - 1:
            if num_update <= self.step[self.cur_step_ind]:
                break
            self.count = self.step[self.cur_step_ind]
            self.cur_step_ind += 1
            self.base_lr *= self.factor
            (self.logger or logger).info("Update[%d]: Change learning rate to %0.5e", num_update, self.base_lr)
        return self.base_lr


def lr_schedule(base_lr, lr_step, begin_epoch, num_pairs, num_gpus=1, lr_factor=0.1):
    """train.py:244-254 → (lr, lr_epoch, lr_epoch_diff, lr_iters): the epochs of TRAIN.lr_step ("4, 6"), those still ahead of
    begin_epoch counted from it, the starting lr (base_lr · lr_factor per boundary already passed) and the boundaries in updates,
    int(epoch · num_pairs / num_gpus). A resumed run counts its updates from 0 again, which is what the subtraction presumes."""
    lr_epoch = [float(epoch) for epoch in str(lr_step).split(",")]
    lr_epoch_diff = [epoch - begin_epoch for epoch in lr_epoch if epoch > begin_epoch]
    lr = base_lr * (lr_factor ** (len(lr_epoch) - len(lr_epoch_diff)))
    lr_iters = [int(epoch * num_pairs / num_gpus) for epoch in lr_epoch_diff]
    return lr, lr_epoch, lr_epoch_diff, lr_iters
