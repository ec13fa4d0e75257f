"""The training loop: MutableModule.fit (deepim/core/module.py:973-1186) over deepIM_flownet.train_step.

A single device, the bound training graph and its device batch updater; the metrics are reduced on the device (core/metric.py),
so inside the batch loop nothing is allocated and nothing is read back except where a line is printed: eval_metric.get() in
Speedometer and at the end of an epoch, and the weight-norm line.

Differences from the reference, all of them stated in INTEGRATION.md:
  * `train_data` is an iterable of (data, label) dicts of device arrays, as lib/pair_matching/data_pair.get_data_pair_train_batch
    returns them (data also carries tgt_pose [, depth_gt_observed, class_index] for the batch updater), with `batch_size` and
    `reset()`. There is no DataIter / DataBatch, no PrefetchingIter, no kvstore and no executor group;
  * the learning rate is evaluated per update as mx.optimizer does: the k-th update since fit began uses lr_scheduler(k), k from
    1, so the TRAIN_ITER_SIZE updates of one batch may straddle a boundary of the schedule;
  * TRAIN.RESUME loads prefix-%04d.params and .states of begin_epoch; the update count restarts at 0, as train.py:247-249 presumes;
  * TRAIN.VISUALIZE, TRAIN.TENSORBOARD_LOG and eval_data are refused.
"""
import collections
import logging
import time

import numpy as np

from ..lib.utils import load_model, ndarray_file
from ..runtime import lib

BatchEndParam = collections.namedtuple("BatchEndParams", ["epoch", "nbatch", "eval_metric", "locals"])


def _as_list(obj):
    return obj if isinstance(obj, (list, tuple)) else [obj]


class MutableModule(object):
    """MutableModule(config, net): `net` is a deepIM_flownet training graph after bind_train."""

    def __init__(self, config, net, logger=None):
        self.config = config
        self.net = net
        self.logger = logger or logging.getLogger(__name__)
        self._norm_table = None

    # -- parameters and checkpoints
    def get_params(self):
        """-> (arg_params, aux_params) as host arrays (the graph has no auxiliary states)."""
        return {k: v.asnumpy() for k, v in self.net.params.items()}, {}

    def save_checkpoint(self, prefix, epoch, save_optimizer_states=False):
        """prefix-%04d.params through lib/utils/load_model.save_checkpoint and, asked for, prefix-%04d.states: the dict of
        deepIM_flownet.optimizer_states() through ndarray_file (Module.save_checkpoint)."""
        arg_params, aux_params = self.get_params()
        load_model.save_checkpoint(prefix, epoch, arg_params, aux_params)
        self.logger.info('Saved checkpoint to "%s-%04d.params"', prefix, epoch)
        if save_optimizer_states:
            ndarray_file.save("%s-%04d.states" % (prefix, epoch), self.net.optimizer_states())
            self.logger.info('Saved optimizer state to "%s-%04d.states"', prefix, epoch)

    def load_checkpoint(self, prefix, epoch, load_optimizer_states=True):
        """Re-bind the graph on prefix-%04d.params (every packed form of the weights is rebuilt) and restore the .states."""
        net = self.net
        arg_params, _aux = load_model.load_checkpoint(prefix, epoch)
        net.bind_train(net.ctx, net.B, arg_params, num_points=net.num_points)
        self._norm_table = None
        if load_optimizer_states:
            net.load_optimizer_states(ndarray_file.load("%s-%04d.states" % (prefix, epoch)))

    # -- the weight-norm line
    def weight_norms(self):
        """-> [(name, 2-norm float32)] over the sorted parameter names: one deepim_l2_norms_multi call, one read-back of a float
        per parameter (module.py:1114-1120 reads every parameter back)."""
        net = self.net
        names = sorted(net.params.keys())
        if self._norm_table is None:
            table = net.ctx.empty((len(names), 2), np.uint64)
            table.copyfrom(np.array([[net.params[n].ptr, net.params[n].size] for n in names], dtype=np.uint64))
            self._norm_table = (table, net.ctx.empty((len(names),), np.float32))
        table, out = self._norm_table
        lib.deepim_l2_norms_multi(net.ctx.handle, out, table, len(names))
        return list(zip(names, out.asnumpy()))

    # -- the loop
    def fit(self, train_data, eval_metric=None, epoch_end_callback=None, batch_end_callback=None, optimizer_params=None,
            begin_epoch=0, num_epoch=None, prefix=None, updater=None, logger=None, eval_data=None):
        """module.py:1086-1186. optimizer_params as train.py builds them: SGD {"learning_rate", "momentum", "wd", "lr_scheduler"}
        (defaults TRAIN.lr / TRAIN.momentum / TRAIN.wd, no scheduler), Adam {"learning_rate"} only (train.py:261: a scheduler
        is ignored, as it is never handed to Adam there). `updater` is the batchUpdaterPyMulti with a device render machine that
        train_step needs between the iterations of a batch."""
        assert num_epoch is not None, "please specify number of epochs"
        config, net = self.config, self.net
        logger = logger or self.logger
        if eval_metric is None:
            from .metric import CompositeEvalMetric
            eval_metric = CompositeEvalMetric()      # no metric: the loop runs, the lines carry no values
        if eval_data is not None:
            raise NotImplementedError("fit: eval_data (deepim/core/module.py:1173-1183, validation scoring) is not part of this port")
        if config.TRAIN.get("VISUALIZE", False):
            raise NotImplementedError("TRAIN.VISUALIZE (deepim/train.py:232-235, deepim/core/metric.py:140-486) draws figures; "
                                      "it is not part of this port")
        if config.TRAIN.get("TENSORBOARD_LOG", False):
            raise NotImplementedError("TRAIN.TENSORBOARD_LOG (deepim/core/module.py:1096-1100, :1123-1129, :1150-1158) needs mxboard; "
                                      "it is not part of this port")
        opt = dict(optimizer_params or {})
        unknown = set(opt) - {"learning_rate", "momentum", "wd", "lr_scheduler", "rescale_grad", "clip_gradient"}
        if unknown:
            raise ValueError("fit: unknown optimizer_params {}".format(sorted(unknown)))
        if opt.get("clip_gradient") is not None or opt.get("rescale_grad", 1.0) != 1.0:
            raise NotImplementedError("fit: rescale_grad / clip_gradient other than train.py:302-303's (1.0, None)")
        adam = net.optimizer == "adam"
        base_lr = opt.get("learning_rate", config.TRAIN.lr)
        scheduler = None if adam else opt.get("lr_scheduler")
        if scheduler is not None:
            scheduler.base_lr = base_lr          # mx.optimizer.Optimizer.__init__
        momentum = None if adam else opt.get("momentum", config.TRAIN.momentum)
        wd = None if adam else opt.get("wd", config.TRAIN.wd)

        if config.TRAIN.get("RESUME", False):
            self.load_checkpoint(prefix, begin_epoch)
        num_update = [0]                         # mx.optimizer's num_update: updates since fit began

        def get_lr(k):
            return base_lr if scheduler is None else scheduler(k)

        def lr_of_iteration(it):
            return get_lr(num_update[0] + it + 1)

        if epoch_end_callback is not None:
            for callback in _as_list(epoch_end_callback):
                callback(-1, net, None, None)

        train_iter_size = int(config.network.TRAIN_ITER_SIZE)
        last_lr = 0
        for epoch in range(begin_epoch, num_epoch):
            tic = time.time()
            eval_metric.reset()
            for nbatch, (data, label) in enumerate(train_data):
                cur_lr = get_lr(num_update[0])
                if nbatch % (4000 / train_data.batch_size) == 0:     # the reference's expression, float division included
                    logger.info("{}".format(prefix))
                    logger.info("".join("{}: {} ".format(name, np.array([v], np.float32)) for name, v in self.weight_norms()))
                    logger.info("batch {}: lr: {}".format(nbatch, cur_lr))
                if cur_lr != last_lr:
                    logger.info("batch {}: lr: {}".format(nbatch, cur_lr))
                    last_lr = cur_lr
                data, label = net.train_step(data, label, updater, iters=train_iter_size, lr=lr_of_iteration, wd=wd,
                                             momentum=momentum)
                num_update[0] += train_iter_size
                eval_metric.update(label, net.train_outputs())       # the last iteration's outputs (module.py:1139)
                if batch_end_callback is not None:
                    param = BatchEndParam(epoch=epoch, nbatch=nbatch, eval_metric=eval_metric, locals=None)
                    for callback in _as_list(batch_end_callback):
                        callback(param)
            for name, val in eval_metric.get_name_value():
                logger.info("Epoch[%d] Train-%s=%f", epoch, name, val)
            toc = time.time()
            logger.info("Epoch[%d] Time cost=%.3f", epoch, (toc - tic))
            if epoch_end_callback is not None:
                for callback in _as_list(epoch_end_callback):
                    callback(epoch, net, None, None)
            train_data.reset()
