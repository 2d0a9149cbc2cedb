"""Derived copies of weights (a bf16 cast, a packed Q|K|V, BatchNorm folded into a convolution) and the one rule for when such a
copy is stale: it is current while `key_of` its sources has not moved -- unless an optimiser that writes parameters through raw
pointers (engine.FlatTrainer's Adam kernel, which moves neither a version nor a pointer) has promised to keep a view current."""
from . import ops


def key_of(tensors):
    """What "has not moved" means: a write through torch bumps `_version`; `.to()`, `p.data = ...` and `load_state_dict(assign=True)`
    move the pointer or the device."""
    return tuple((t._version, t.data_ptr(), t.device) for t in tensors)


class Cached:
    """A value derived from many tensors: `build()` runs again when `key_of(sources())` has changed."""

    def __init__(self, sources, build):
        self.sources, self.build = sources, build
        self._key, self._value = None, None

    def get(self):
        key = key_of(self.sources())
        if key != self._key:
            self._value, self._key = self.build(), key
        return self._value

    def invalidate(self):
        self._key = None


class Bf16Weight:
    """The bf16 copy of one fp32 parameter, as the MFMA kernels read it."""

    def __init__(self, param):
        self.param = param
        self._own, self._key = None, None  # this object's copy, and its key when it was cast
        self._view, self._ptr, self._version = None, None, None  # the attachment: the owner's view, param's pointer, the version seen

    def get(self):
        p = self.param
        if self._view is not None and p.data_ptr() == self._ptr:
            if p._version != self._version:  # written through torch (load_state_dict, an in-place op): refresh the view itself
                ops.cast_bf16(p.detach().contiguous(), self._view)
                self._version = p._version
            return self._view
        # not attached, or the parameter moved and the attachment is void.  Cast in place while shape and device stand: captured
        # graphs and decode sessions hold this pointer
        key = (p._version, p.data_ptr(), p.device)  # key_of, written out for the one tensor: this runs per matrix and forward
        if key != self._key:
            keep = self._own is not None and self._own.shape == p.shape and self._own.device == p.device
            self._own = ops.cast_bf16(p.detach().contiguous(), self._own if keep else None)
            self._key = key
        return self._own

    def attach(self, view):
        """The owner promises to keep `view` == bf16(param) for as long as param.data_ptr() stays where it is now."""
        self._view, self._ptr, self._version = view, self.param.data_ptr(), self.param._version
        self._own, self._key = None, None

    def mark_fresh(self):
        """The owner has just written the view to match the parameter (nothing to do when nothing is attached)."""
        if self._view is not None:
            self._version = self.param._version

    def invalidate(self):
        """Drop the attachment and the key: the next get() casts."""
        self._view, self._key = None, None
