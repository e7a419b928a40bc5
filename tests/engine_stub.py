"""A stand-in for the HIP library under diffrl_amd.engine.Engine, for the CPU tier: Engine._call is the only method that touches
torch.cuda, so a subclass whose _call RECORDS what it is handed -- the function's name, the scalars, and for every pointer either
None or the tensor behind it (its role, numel, dtype, shape) -- drives the whole binding layer without loading or launching
anything.  tests/test_engine_binding_cpu.py is its user."""
import contextlib
import ctypes as C

import torch

CKPT_ROW, CKPT_HINV, LITERAL_SCRATCH = 256, 16, 24   # what the two size queries of the fake library answer with


class _Fn:
    """a function of the fake library: a name to record"""

    def __init__(self, name):
        self.name = name

    def __call__(self, *args):
        raise AssertionError("%s was called directly: a launch goes through Engine._call" % self.name)


class FakeLib:
    def dsim_ckpt_floats_mm(self, h, substeps, mm_freq):
        return substeps * CKPT_ROW + -(-substeps // mm_freq) * CKPT_HINV

    def dsim_literal_scratch_floats(self, h):
        return LITERAL_SCRATCH

    def __getattr__(self, name):
        return _Fn(name)


def stub_class(engine_module):
    """the recording subclass of engine_module.Engine (diffrl_amd.engine, or another version of that file)"""

    class Stub(engine_module.Engine):
        module = engine_module

        def __init__(self, template, ckpt_mode="full"):   # (never Engine.__init__: that one loads the library and creates a model)
            self.template, self.device, self.ckpt_mode = template, torch.device("cpu"), ckpt_mode
            self._lib, self._h = FakeLib(), "model"
            self.n_q, self.n_qd, self.n_muscles = template.n_q, template.n_qd, template.n_muscles
            self.last_q_in = None
            self.calls, self.roles = [], {}

        def __del__(self):
            pass

        def T(self, role, *shape, dtype=torch.float32):
            """a tensor to hand in, known to the record as `role` from here on (by its storage: a detached alias is the same)"""
            t = (torch.arange(int(torch.Size(shape).numel()), dtype=torch.float32).reshape(shape) * 0.01 + 0.5).to(dtype)
            self.roles[t.data_ptr()] = (role, t)   # (kept alive: its address is not handed out again while the stub lives)
            return t

        def _describe(self, a):
            if isinstance(a, torch.Tensor):   # "new": allocated on the way, by the engine or an autograd function
                role = self.roles.get(a.data_ptr(), ("new",))[0] if a.numel() else "empty"
                return [role, a.numel(), str(a.dtype), list(a.shape)]
            if isinstance(a, C.c_float):
                return round(float(a.value), 9)
            if hasattr(a, "_obj"):   # byref(spec), byref(episode): the structure's name, its integers, which pointers are set
                s = a._obj
                return [type(s).__name__] + [[f, getattr(s, f) if t in (C.c_int32,) else getattr(s, f) is not None]
                                             for f, t in s._fields_ if t in (C.c_int32, C.c_void_p)]
            return a   # None, an int, the model handle

        def _call(self, fn, *args):
            self.calls.append([fn.name] + [self._describe(a) for a in args])

    return Stub


@contextlib.contextmanager
def recording(stub):
    """within it, the engine module hands _call the tensors themselves instead of their addresses (its _ptr is the identity),
    and stub.calls starts empty"""
    m = stub.module
    keep, m._ptr = m._ptr, lambda t: t
    stub.calls = []
    try:
        yield stub.calls
    finally:
        m._ptr = keep
