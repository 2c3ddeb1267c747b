"""What rides the step (new; the reference has none): the protocol between FluidSimulator and the objects whose launches go behind every
solver step - fs.history.Recorder, fs.averages.Averager, fs.modes.Modes, fs.pod.Pod, fs.dist.Distributions, fs.spectra.Spectra, fs.spectra.CrossSpectra, fs.fluxes.ScaleFluxes, fs.budgets.Budget, fs.loads.Tracker, fs.tracers.Tracers, fs.vortices.Vortices, in the order of fs.fluid_simulator.RIDER_ATTRS -, the base of those that
accumulate over counted samples (CountedRider) and the one host-side sampling rule.
DESIGN.md "Riders" says what a new rider has to implement, and what a new CountedRider has to state."""
import collections
import operator

import numpy as np


def is_sampling_launch(n, every, start):
    """Whether launch n (counted from 0) samples: n + 1 > start and (n + 1 - start) % every == 0 (csrc/fs_device.h samples_at)."""
    return n + 1 > start and (n + 1 - start) % every == 0


def samples_after(launches, every, start):
    """Samples taken by the first `launches` launches."""
    return max(0, (int(launches) - int(start)) // int(every))


def ring_room(issued, every, start, capacity, gone):
    """Launches that may follow `issued` before a sampling one would find a ring of `capacity` records full; `gone`: the samples that are
    not in the ring any more (drained, or taken before it existed)."""
    return start + (capacity + gone + 1) * every - 1 - issued


class Rider:
    """One attachment of a FluidSimulator.  FluidSimulator._riders() yields the attached ones in the fixed order of
    fs.fluid_simulator.RIDER_ATTRS: the order of their launches behind the solver step and of their tokens in _signature()."""
    stop_in_capture = True       # stop_*() inside a graph capture: allowed (the device memory goes when the capture ends), or RuntimeError
    keeps_last = False           # stop_*() keeps the rider as sim._last_*: its readers go on returning what it gathered
    replaces_attached = False    # attaching while one of the kind is attached: stops that one first, or RuntimeError
    issued = 0                   # launches issued (captured launches count when their capture runs once)

    def tokens(self):
        """What _signature() holds for this rider: graphs / tapes with its launches in them are never replayed without it, or vice versa."""
        return (self.token,)

    def launch(self, sim):
        """Issue the launches behind one solver step and count them; a rider with a ring drains it first when it is full (eager steps
        beyond the ring: run() drains between its chunks instead)."""
        raise NotImplementedError

    def _make_room(self):
        if self.room() <= 0 and not getattr(self.dev, "capturing", False):
            self.drain()

    def replayed(self, steps):
        self.issued += steps

    def room(self):
        """Steps that may run before a device ring would be full; None: no ring."""
        return None

    def drain(self):
        """Empty the ring into host memory."""

    def next_cut(self):
        """Steps until run() has to end a chunk for between_chunks() (>= 1); None: never."""
        return None

    def between_chunks(self):
        """Between two launch sequences (after an eager step, between run()'s chunks), never inside a capture."""

    def close(self):
        """Before free() of a rider that keeps_last: fetch what its readers need once the device object is gone."""

    def free(self):
        """Release the device objects."""
        raise NotImplementedError

    def checkpoint(self):
        """{checkpoint key: array} of everything a resumed run needs."""
        return {}

    @staticmethod
    def held(z):
        """The parameters the checkpoint mapping z holds under this rider's keys, or None when it holds none of its kind: what a caller
        compares with its own before restore()."""
        return None

    def restore(self, z):
        """The inverse of checkpoint() on a freshly attached rider with the same parameters; z: the checkpoint's mapping -> the samples
        taken over."""


class Param(collections.namedtuple("Param", "key write read refusal same", defaults=(operator.eq,))):
    """One parameter a CountedRider is attached with: `key` of its checkpoint entry (behind the kind's prefix), `write` the attached value
    -> the array stored there, `read` that array -> the value held() returns and restore() compares (`same`) with the attached one, and
    `refusal`, the words of restore()'s ValueError when they differ: a format of {theirs} ("the checkpoint's <noun> was / were"), {ours}
    ("the attached one / ones"), {0} the checkpoint's value and {1} the attached one."""
    __slots__ = ()


def _ints(a):
    return tuple(int(b) for b in np.asarray(a))


BOX = Param("box", lambda box: np.array(box, np.int64), _ints, "{theirs} accumulated over the box {0}, {ours} over {1}")


class CountedRider(Rider):
    """A rider that accumulates over counted samples: one device object `obj` holding (payload, launches, samples), reached through the
    calls dev.<kind>_read / _get / _set / _reset / _free, and `base`, the samples taken before the last reset.  No ring: room() is None and
    run() is not cut by it.  A subclass states `kind` (the stem of those calls, the prefix of its checkpoint keys, its token), `payload` (the
    key of the payload), `noun` and `plural` (how restore()'s refusals call it), `params` (Param, in the order they are compared) with
    attached() - their attached values -, launch(sim) and data()."""
    kind = payload = noun = None
    plural = False
    params = ()
    refuses_missing = True       # restore() of a checkpoint without this kind: ValueError "the checkpoint holds no <noun>", or the KeyError of its first key

    def __init__(self, dev, obj, every, start_step):
        self.dev, self.obj, self.every, self.start_step = dev, obj, int(every), int(start_step)
        self.base = 0              # samples taken before the last reset (sample_steps)
        self.token = (self.kind, obj.serial)

    def _call(self, what, *args, **kw):
        return getattr(self.dev, f"{self.kind}_{what}")(self.obj, *args, **kw)

    def attached(self):
        """The attached values of `params`, in their order."""
        return ()

    def free(self):
        self._call("free")

    def sample_steps(self, samples):
        """The step (counted from the call that attached the rider, from 1) of every sample accumulated, int64 (samples,)."""
        k = self.base + np.arange(int(samples), dtype=np.int64)
        return self.start_step + (k + 1) * self.every

    def _launches(self):
        return self._call("read", **{self.payload: False})[1]

    def reset(self):
        launches = self._launches()
        self._call("reset")
        self.base = samples_after(launches, self.every, self.start_step)

    def checkpoint(self):
        k = self.kind
        payload, launches, samples = self._call("get")
        out = {f"{k}.{self.payload}": payload, f"{k}.launches": np.array(launches), f"{k}.samples": np.array(samples),
               f"{k}.base": np.array(self.base), f"{k}.every": np.array(self.every), f"{k}.start": np.array(self.start_step)}
        out.update((f"{k}.{p.key}", p.write(mine)) for p, mine in zip(self.params, self.attached()))
        return out

    @classmethod
    def _held(cls, z):
        k = cls.kind
        return tuple(p.read(z[f"{k}.{p.key}"]) for p in cls.params) + (int(z[f"{k}.every"]), int(z[f"{k}.start"]))

    @classmethod
    def held(cls, z):
        """-> (the value of every one of `params`, every, start), or None."""
        return cls._held(z) if f"{cls.kind}.{cls.payload}" in z else None

    def restore(self, z):
        """Refused (ValueError) before any device work when a parameter, every or start_step of the checkpoint's are not the attached
        ones."""
        k = self.kind
        if self.refuses_missing and self.held(z) is None:
            raise ValueError(f"the checkpoint holds no {self.noun}")
        *held, every, start = self._held(z)
        theirs = f"the checkpoint's {self.noun} {'were' if self.plural else 'was'}"
        ours = "the attached ones" if self.plural else "the attached one"
        for p, value, mine in zip(self.params, held, self.attached()):
            if not p.same(value, mine):
                raise ValueError(p.refusal.format(value, mine, theirs=theirs, ours=ours))
        if (every, start) != (self.every, self.start_step):
            raise ValueError(f"the checkpoint's {self.noun} sample{'' if self.plural else 's'} every {every} from {start}, {ours} every "
                             f"{self.every} from {self.start_step}")
        self._call("set", z[f"{k}.{self.payload}"], int(z[f"{k}.launches"]), int(z[f"{k}.samples"]))
        self.base = int(z[f"{k}.base"])
        return int(z[f"{k}.samples"])
