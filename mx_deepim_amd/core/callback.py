"""Training callbacks: Speedometer (deepim/core/callback.py:11-42) and the per-epoch checkpoint train.py:242 asks of
mx.callback.module_checkpoint(mod, prefix, period=1, save_optimizer_states=True)."""
import logging
import time

logger = logging.getLogger(__name__)


class Speedometer(object):
    """Batch-end callback: every `frequent` batches one line with the samples per second since the last line and the current
    value of every metric — the reference's text, character for character. It takes an object with `epoch`, `nbatch` and
    `eval_metric`. eval_metric.get() is the loop's one read-back of the metric sums."""

    def __init__(self, batch_size, frequent=50, logger=None):
        self.batch_size = batch_size
        self.frequent = frequent
        self.init = False
        self.tic = 0
        self.last_count = 0
        self.logger = logger

    def __call__(self, param):
        count = param.nbatch
        if self.last_count > count:       # a new epoch: the first batch only starts the clock
            self.init = False
        self.last_count = count
        if not self.init:
            self.init = True
            self.tic = time.time()
            return
        if count % self.frequent != 0:
            return
        speed = self.frequent * self.batch_size / (time.time() - self.tic)
        if param.eval_metric is not None:
            names, values = param.eval_metric.get()
            s = "Epoch[%d] Batch [%d]\tSpeed: %.2f samples/sec\tTrain-" % (param.epoch, count, speed)
            for n, v in zip(names, values):
                s += "%s=%f,\t" % (n, v)
        else:
            s = "Iter[%d] Batch [%d]\tSpeed: %.2f samples/sec" % (param.epoch, count, speed)
        (self.logger or logger).info(s)
        self.tic = time.time()


def module_checkpoint(mod, prefix, period=1, save_optimizer_states=True):
    """Epoch-end callback (mx.callback.module_checkpoint): after epoch `iter_no`, when (iter_no + 1) % period == 0, write
    prefix-%04d.params [and .states] numbered iter_no + 1 through mod.save_checkpoint. So the call with -1 that fit makes
    before the first epoch writes prefix-0000.*."""
    period = int(max(1, period))

    def _callback(iter_no, sym=None, arg=None, aux=None):
        if (iter_no + 1) % period == 0:
            mod.save_checkpoint(prefix, iter_no + 1, save_optimizer_states)

    return _callback
