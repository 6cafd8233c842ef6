"""mbx_plan_bitmap_form at the C-ABI boundary: declared by include/mbx.h,
exported by libmbx.so, listed by the Python binding, and refusing null
arguments before it touches a device (no GPU needed)."""
import ctypes
import os
import re

import helpers
import mbx_pkg

NAME = "mbx_plan_bitmap_form"


def test_header_declares_it():
    src = open(os.path.join(helpers.ROOT, "include", "mbx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"^\s*int\s+%s\s*\(\s*mbx_ctx\s*\*\s*\w+\s*,\s*const\s+mbx_plan\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;"
                     % NAME, src, flags=re.M)


def test_library_exports_it():
    so = ctypes.CDLL(os.path.join(mbx_pkg.PKG_DIR, "libmbx.so"))
    assert hasattr(so, NAME)


def test_binding_lists_it():
    m = mbx_pkg.load()
    assert NAME in m.mbx.EXPORTS
    assert callable(getattr(m.Context, "plan_bitmap_form"))


def test_null_arguments_are_rejected_without_a_device():
    m = mbx_pkg.load()
    L = m.lib()
    fn = getattr(L, NAME)
    form = ctypes.c_int32(-7)
    # a null argument is refused before any argument is read: the stand-in handles are never followed
    standin = ctypes.create_string_buffer(64)
    h = ctypes.c_void_p(ctypes.addressof(standin))
    for args, which in (((None, h, ctypes.byref(form)), b"c"), ((h, None, ctypes.byref(form)), b"p"),
                        ((h, h, None), b"form"), ((None, None, None), b"c")):
        assert fn(*args) == m.mbx.E_INVALID
        err = L.mbx_last_error()
        assert b"null" in err and NAME.encode() in err and b"`" + which + b"`" in err, err
    assert form.value == -7
