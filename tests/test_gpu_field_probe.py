"""The DEVICE branches of the field primitives, one op per test, one operand class per case (p3hip_field_probe_dev against
tests/field_ref.py).  Integer and extension ops: the device words equal the reference.  fp64 ops: the device doubles equal the exact
model as numbers (==, so -0.0 passes): a mismatch means the compiler did not keep the operations as written, or the model is wrong.
One launch per op, shared by its cases; the largest is the extension pair grid, 407 009 lanes."""
import ctypes as C

import numpy as np
import pytest

import field_ref as F

pytestmark = pytest.mark.gpu
P = F.P
_results = {}


def probe_dev(name, x):
    import torch
    from plonky3_mobile_amd import _lib
    op, k, m, f64 = F.OPS[name]
    x = np.array(x, copy=True, order="C")  # the cached lanes are read-only
    assert x.ndim == 2 and x.shape[1] == k and len(x) <= 1 << 20 and x.dtype == (np.float64 if f64 else np.uint32)
    d = torch.from_numpy(x.view(np.int32) if not f64 else x).cuda()
    out = torch.zeros((len(x), m), dtype=torch.float64 if f64 else torch.int32, device="cuda")
    _lib.check(_lib.lib().p3hip_field_probe_dev(op, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), len(x),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    r = out.cpu().numpy()
    return r if f64 else r.view(np.uint32)


def device(p3, name):
    if name not in _results:
        _results[name] = probe_dev(name, F.lanes(name)[0])
    return _results[name]


def _check(p3, name, cls):
    x, lab = F.lanes(name)
    sel = np.flatnonzero(lab == cls)
    assert sel.size >= F.MIN_LANES
    got, want = device(p3, name)[sel], F.expected(name)[sel]
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, "%d of %d lanes differ; first: %r" % (
        bad.size, sel.size, [(x[sel[i]].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:4]])


def _make(name):
    @pytest.mark.parametrize("cls", F.CLASSES[name], ids=[F.class_id(c) for c in F.CLASSES[name]])
    def test(p3, cls):
        _check(p3, name, cls)
    test.__name__ = test.__qualname__ = "test_" + name
    test.__doc__ = "%s, op %d: device result against the %s, class by class" % (name, F.OPS[name][0], "exact model" if F.OPS[name][3] else "reference")
    return test


for _name in F.OPS:
    globals()["test_" + _name] = _make(_name)
del _name


def test_extension_inverse_times_element_is_one(p3):
    """a * inv(a) = 1 ON THE DEVICE for every nonzero lane of the inverse's classes (the grid, 2^16 random elements, the structural
    classes), and inv(0) = 0."""
    x, _ = F.lanes("ext_inv")
    inv = device(p3, "ext_inv")
    prod = probe_dev("ext_mul", np.concatenate([x, inv], axis=1))
    nz = np.any(x != 0, axis=1)
    assert np.all(prod[nz] == np.array([F.ONE, 0, 0, 0], np.uint32)) and np.all(inv[~nz] == 0) and np.all(prod[~nz] == 0)


def test_two_adic_generator_orders(p3):
    """g = two_adic_generator(b): g^(2^b) = 1 and g^(2^(b-1)) = -1, with the device's own pow."""
    g = device(p3, "two_adic_generator")[:28]
    bits = F.lanes("two_adic_generator")[0][:28, 0]
    assert bits.tolist() == list(range(28))
    full = probe_dev("pow", np.array([(int(w), (1 << b) & F.M32, 0) for w, b in zip(g[:, 0], bits)], np.uint32))
    half = probe_dev("pow", np.array([(int(w), (1 << b >> 1) & F.M32, 0) for w, b in zip(g[:, 0], bits)], np.uint32))
    assert np.all(full[:, 0] == F.ONE) and half[0, 0] == F.ONE and np.all(half[1:, 0] == P - F.ONE)


def test_device_probe_refuses_bad_arguments(p3):
    import torch
    from plonky3_mobile_amd import _lib
    lib = _lib.lib()
    d = torch.zeros(8, dtype=torch.float64, device="cuda")
    ptr = C.c_void_p(d.data_ptr())
    for op in (0, 21, 31, 44):
        assert lib.p3hip_field_probe_dev(op, ptr, ptr, 1, None) == -1 and "unknown op %d" % op in p3.take_last_error()
    assert lib.p3hip_field_probe_dev(1, ptr, ptr, (1 << 22) + 1, None) == -1 and "2^22" in p3.take_last_error()
    assert lib.p3hip_field_probe_dev(1, None, ptr, 1, None) == -1 and "null" in p3.take_last_error()
    assert lib.p3hip_field_probe_dev(1, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert d.cpu().tolist() == [0.0] * 8
