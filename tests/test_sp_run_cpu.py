"""CPU: the host side of batched stand-alone Spatial Pooler runs (SpatialPooler.run, Engine.sp_run, htm_sp_run): the C
declaration and the record structure against the binding, the refusals that need no device, and how `record=` is parsed."""

import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


C_TYPES = {"htm_handle *": C.c_void_p, "const uint32_t *": C.c_void_p, "int32_t": C.c_int32}


def _header():
    return open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()


def test_header_declares_htm_sp_run_as_the_binding_calls_it(built):
    from bithtm_amd import _lib
    m = re.search(r"^int htm_sp_run\(([^)]*)\);", _header(), flags=re.M)
    assert m, "include/bithtm_hip.h does not declare htm_sp_run"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    types = [p[:-len(n)].strip() for p, n in zip(params, names)]
    assert names == ["h", "device_inputs", "n_inputs", "n_steps", "learning", "use_graph", "rec"]
    want = [C.POINTER(_lib.HtmSpRunRecord) if t == "const htm_sp_run_record *" else C_TYPES[t] for t in types]
    restype, argtypes = _lib.EXPORTS["htm_sp_run"]
    assert restype is C.c_int and argtypes == want
    lib = _lib.load()
    assert lib.htm_sp_run.argtypes == want
    assert lib.htm_sp_run(None, None, 1, 1, 1, 1, None) == -1              # a NULL handle: HTM_ERR_ARGUMENT, nothing touched


def test_record_structure_matches_the_header(built):
    from bithtm_amd import _lib
    from bithtm_amd.engine import SP_RECORD_FIELDS
    m = re.search(r"typedef struct htm_sp_run_record \{(.*?)\} htm_sp_run_record;", _header(), flags=re.S)
    assert m, "include/bithtm_hip.h does not define htm_sp_run_record"
    fields = re.findall(r"^\s*([\w ]+?)\s*(\*?)\s*(\w+);", m.group(1), flags=re.M)
    assert [(t.strip(), star, name) for t, star, name in fields] == [
        ("uint32_t", "", "struct_bytes"), ("int32_t", "*", "active_column"), ("int32_t", "*", "active_overlap"), ("double", "*", "active_boosted")]
    # a 64-bit ABI: the 4-byte word, 4 bytes of padding in front of the first pointer, three pointers
    size, offset = 0, {}
    for _, star, name in fields:
        width = 8 if star else 4
        size = -(-size // width) * width
        offset[name] = size
        size += width
    assert size == 32 == C.sizeof(_lib.HtmSpRunRecord)
    assert [name for name, _ in _lib.HtmSpRunRecord._fields_] == [name for _, _, name in fields]
    for name, _ in _lib.HtmSpRunRecord._fields_:
        assert getattr(_lib.HtmSpRunRecord, name).offset == offset[name], name
    assert tuple(name for name, _ in _lib.HtmSpRunRecord._fields_[1:]) == SP_RECORD_FIELDS


def test_run_refuses_on_the_host_before_any_engine_exists(built):
    import bithtm_amd as B
    I, Cn, k = 40, 64, 4
    inputs = np.random.RandomState(0).rand(3, I) < 0.2
    sp = B.SpatialPooler(I, Cn, k)
    for kw, what in ((dict(steps=-1), "negative"),
                     (dict(inputs=inputs[0]), "inputs"), (dict(inputs=inputs[:, :-1]), "inputs"), (dict(inputs=inputs[:0]), "inputs"),
                     (dict(inputs=inputs[None]), "inputs"),
                     (dict(record=("nonsense",)), "record"), (dict(record=("active_column", "counters")), "record"), (dict(record=()), "record"),
                     (dict(noise=-0.01), "noise"), (dict(noise=1.5), "noise"), (dict(noise=float("nan")), "noise"), (dict(noise=[0.1, 0.2]), "noise"),
                     (dict(steps=(1 << 32) + 1), r"2\^32")):
        with pytest.raises(ValueError, match=what):
            sp.run(**{**dict(inputs=inputs, steps=4), **kw})
        assert sp._engine is None                               # nothing was created, let alone enqueued

    class Projection(B.DenseProjection):
        pass
    plug = B.SpatialPooler(I, Cn, k, proximal_projection=Projection(I, Cn))
    with pytest.raises(ValueError, match=r"call process\(\)"):
        plug.run(inputs, 4)
    assert plug._engine is None
    fused = B.SpatialPooler(I, Cn, k)
    fused._fused = True                                         # (what HierarchicalTemporalMemory's constructor leaves on its pooler)
    with pytest.raises(ValueError, match=r"call its run\(\)"):
        fused.run(inputs, 4)
    assert fused._engine is None


def test_record_argument_parsing(built):
    import bithtm_amd as B
    from bithtm_amd.networks import _sp_record_fields
    assert _sp_record_fields(True) == ("active_column",)
    assert _sp_record_fields("active_boosted") == ("active_boosted",)
    assert _sp_record_fields(("active_boosted", "active_column")) == ("active_column", "active_boosted")
    assert _sp_record_fields(["active_overlap", "active_overlap", "active_column"]) == ("active_column", "active_overlap")
    assert _sp_record_fields(("active_boosted", "active_overlap", "active_column")) == ("active_column", "active_overlap", "active_boosted")
    for bad in ((), "counters", ("active_column", "predicted_input"), ""):
        with pytest.raises(ValueError, match="record"):
            _sp_record_fields(bad)
    rec = B.SPRunRecord(np.arange(3) + 5, active_overlap=np.zeros((3, 2), np.int32))
    assert rec.fields == ("active_overlap",) and rec.active_column is None and rec.active_boosted is None and len(rec) == 3
    assert rec.step_index.dtype == np.int64 and rec.step_index.tolist() == [5, 6, 7]
