"""Scheduled sampling (Bengio et al. 2015; include/lrcn_sched.h) around the trainer: the epsilon schedule and the per-step seed.

The device part is lrcn.loss / lossgradient / train_step(..., sched=) and DataParallelTrainer.step(..., sched=); this module is host
arithmetic only and imports nothing that needs a GPU."""


def epsilon(epoch, start, every, step, maximum):
    """Probability of feeding the model's own word in `epoch` (0-based): 0 before `start` (start < 0: never), then
    min(maximum, step * (1 + (epoch - start) // every)) -- raised by `step` every `every` epochs, the schedule of neuraltalk2."""
    epoch, start, every = int(epoch), int(start), int(every)
    if every < 1:
        raise ValueError("every=%d must be >= 1" % every)
    if not 0.0 <= float(maximum) <= 1.0 or float(step) < 0.0:
        raise ValueError("step=%r must be >= 0 and maximum=%r in [0, 1]" % (step, maximum))
    if start < 0 or epoch < start:
        return 0.0
    return min(float(maximum), float(step) * (1 + (epoch - start) // every))


def epoch_seed(seed, epoch):
    """The Philox key an epoch's step seeds start from: a 64-bit mix (splitmix64) of the run's seed and the epoch, the same on every rank
    (the ranks' rows differ through row0)."""
    z = ((int(seed) & 0xFFFFFFFF) << 32 | (int(epoch) & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
    z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def step_seed(epoch_seed_, k):
    """The key of step k of an epoch (train.train1)."""
    return (int(epoch_seed_) + int(k) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def sched_of(start, every, step, maximum, temperature=1.0, seed=0):
    """The `sched_of(epoch)` callable of train.train (epoch 0-based): None while epsilon is 0 (the time-batched calls, untouched), else
    (eps, temperature, the epoch's seed)."""
    def f(epoch):
        eps = epsilon(epoch, start, every, step, maximum)
        return None if eps <= 0.0 else (eps, float(temperature), epoch_seed(seed, epoch))
    return f
