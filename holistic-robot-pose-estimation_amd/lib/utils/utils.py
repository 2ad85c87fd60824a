"""``get_scheduler`` of the reference's lib/utils/utils.py:147-189: the learning-rate schedule of its trainers
(scripts/train_full.py:50, 108 and the other ``train_*.py``: ``lr_scheduler.step()`` once per epoch, after the epoch's
optimizer steps), a ``LambdaLR`` over the optimizer's groups.

Same name, arguments and return value.  The multiplier of the initial rate at epoch ``e``, from the config keys the shipped
YAMLs carry (``n_epochs_warmup``, ``start_decay``, ``end_decay`` and ``final_decay`` / ``exponent`` / ``step``, ``step_decay``):

``linear``       warm-up ``(e + 1) / n_epochs_warmup`` while ``e < n_epochs_warmup``; 1 up to ``start_decay``; then the straight line
                 from 1 at ``start_decay`` to ``final_decay`` at ``end_decay``; ``final_decay`` after it.
``exponential``  the same warm-up and plateau; ``exponent ** (e - start_decay)`` up to ``end_decay``, held at its last value after.
``everyXepoch``  ``step_decay ** (e // step)``, held at ``step_decay ** (end_decay // step)`` from ``end_decay`` on (no warm-up).

``use_schedule: False`` gives ``None``.  With ``use_schedule`` on and a ``schedule_type`` that is none of the three, the reference
reaches its ``return`` with the name unbound and raises ``UnboundLocalError``; that is kept (the test pins it).

The one addition: the scheduler calls ``optimizer.publish_hyper()`` at the end of ``step()`` when the optimizer has that method
(``hrpe_amd.optim.FusedClipAdam``), so the reference's loop line ``lr_scheduler.step()`` also reaches a step that is replayed from a
captured HIP graph.  The rest of the reference's module (data loaders, logger, checkpoint files) is not mirrored here.
"""
import torch


class PublishingLambdaLR(torch.optim.lr_scheduler.LambdaLR):
    """``LambdaLR`` whose ``step()`` ends by handing the new rates to the device (``FusedClipAdam.publish_hyper``)."""

    def step(self, *args, **kwargs):
        out = super().step(*args, **kwargs)
        publish = getattr(self.optimizer, "publish_hyper", None)
        if publish is not None:
            publish()
        return out


def _ratio_linear(args):
    def ratio(epoch):
        if epoch < args.n_epochs_warmup:
            return float(epoch + 1) / float(args.n_epochs_warmup)
        if epoch <= args.start_decay:
            return 1.0
        if epoch > args.end_decay:
            return args.final_decay
        span = float(args.end_decay - args.start_decay)
        # the line through (start_decay, 1) and (end_decay, final_decay), in the reference's association (fp64, bit for bit)
        return (float(args.end_decay - args.final_decay * args.start_decay) - float(1 - args.final_decay) * epoch) / span
    return ratio


def _ratio_exponential(args):
    def ratio(epoch):
        if epoch < args.n_epochs_warmup:
            return float(epoch + 1) / float(args.n_epochs_warmup)
        if epoch <= args.start_decay:
            return 1.0
        return args.exponent ** (min(epoch, args.end_decay) - args.start_decay)
    return ratio


def _ratio_every_x_epoch(args):
    def ratio(epoch):
        return args.step_decay ** ((args.end_decay if epoch >= args.end_decay else epoch) // args.step)
    return ratio


_RATIOS = {"linear": _ratio_linear, "exponential": _ratio_exponential, "everyXepoch": _ratio_every_x_epoch}


def get_scheduler(args, optimizer, last_epoch):
    if not args.use_schedule:
        return None
    if args.schedule_type not in _RATIOS:
        raise UnboundLocalError(f"get_scheduler: unknown schedule_type {args.schedule_type!r} "
                                f"(the reference leaves lr_scheduler unbound); one of {sorted(_RATIOS)}")
    return PublishingLambdaLR(optimizer=optimizer, lr_lambda=_RATIOS[args.schedule_type](args), last_epoch=last_epoch)
