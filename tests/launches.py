"""The one way a test watches op/_native's launch brackets (not a conftest: plain helpers, imported by name).

The observer is process state, so it is installed only through observed(), which puts the null observer back whatever
the body does."""
import contextlib


class Recorder:
    """Launch observer: `seen` holds the (name, info) of every bracket begun, in order."""

    def __init__(self, wants_paths=False):
        self.wants_paths = wants_paths          # True: _native also notes the fused blur's kernel id (BLUR_PATHS)
        self.seen = []

    def begin(self, name, info):
        self.seen.append((name, info))

    def end(self, token):
        pass

    @property
    def names(self):
        return [name for name, _ in self.seen]

    def count(self, name):
        return self.names.count(name)

    def infos(self, name):
        return [info for n, info in self.seen if n == name]


@contextlib.contextmanager
def observed(recorder=None, wants_paths=False):
    """Installs `recorder` (a fresh Recorder by default) for the block and yields it."""
    from op import _native
    rec = Recorder(wants_paths) if recorder is None else recorder
    _native.set_observer(rec)
    try:
        yield rec
    finally:
        _native.set_observer(None)
