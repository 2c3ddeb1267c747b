"""What rides the step (new; the reference has none): the protocol between FluidSimulator and the objects whose launches go behind every
solver step - fs.history.Recorder, fs.averages.Averager, fs.modes.Modes, fs.pod.Pod, fs.dist.Distributions, fs.spectra.Spectra, fs.spectra.CrossSpectra, fs.fluxes.ScaleFluxes, fs.budgets.Budget, fs.loads.Tracker, fs.tracers.Tracers, fs.vortices.Vortices - and the one host-side
sampling rule.
DESIGN.md "Riders" says what a new rider has to implement."""


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
    """One attachment of a FluidSimulator.  FluidSimulator._riders() yields the attached ones in the fixed order history, averages, modes,
    pod, distributions, spectra, cross-spectra, scale fluxes, budget, loads, tracers, vortices: the order of their launches behind the solver step and of their tokens in _signature()."""
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
