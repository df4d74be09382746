"""The C-ABI library loads and exports every symbol include/*.h declares (no GPU)."""
import ctypes
import glob
import os
import re

from nesie_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = open(h).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names += re.findall(r"\b(nesie_[a-z0-9_]+)\s*\(", text)
    return sorted(set(names))


def test_header_declares_the_reference_entry_points():
    names = declared_symbols()
    for stem in ["furthest_point_sampling_wrapper", "furthest_point_sampling_with_dist_wrapper",
                 "ball_query_wrapper", "group_points_forward", "group_points_backward",
                 "gather_points_wrapper", "gather_points_grad_wrapper", "three_nn_wrapper",
                 "three_interpolate_wrapper", "three_interpolate_grad_wrapper",
                 "sort_vertices_forward", "points_in_boxes_batch"]:
        assert "nesie_" + stem in names


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"


def test_binding_is_derived_for_every_declared_function():
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == list(argtypes), name
    assert lib.nesie_abi_version() >= 1
    assert isinstance(lib.nesie_last_error(), bytes)


# The referee: prototypes transcribed by hand from include/*.h, one letter per parameter
# (I int, F float, D double, L long long, Z size_t, P any pointer; the stream is a pointer).
_CODES = {"I": ctypes.c_int, "F": ctypes.c_float, "D": ctypes.c_double, "L": ctypes.c_longlong,
          "Z": ctypes.c_size_t, "P": ctypes.c_void_p}
HAND_WRITTEN = {
    # (int b, n, m, float min_radius, max_radius, int nsample, const float *new_xyz,
    #  const void *fps_workspace, size_t workspace_bytes, int *idx, void *stream)
    "nesie_ball_query_indexed": (ctypes.c_int, "IIIFFIPPZPP"),
    # (int nb, ng, k, cout, long long p, x, long long x_bstride, w, long long w_gstride,
    #  int w_rstride, w_cstride, in_coef, int in_relu, row_bias, int rb_group, bias, y,
    #  long long y_bstride, stat_part, int pool_group, pool_min, float *pool_max_out, pool_min_out,
    #  uint8_t *arg_max_out, arg_min_out, void *stream)
    "nesie_pw_layer_forward": (ctypes.c_int, "IIIIL" "PLPL" "II" "PIPIPP" "LP" "II" "PPPP" "P"),
    # (int nb, ng, co, ci, long long p, dy, long long dy_bstride, x, long long x_bstride, x_coef,
    #  int x_relu, float *dw, void *workspace, size_t workspace_bytes, int defer, void *stream)
    "nesie_pw_wgrad": (ctypes.c_int, "IIIIL" "PLPL" "PIP" "PZ" "I" "P"),
    # (int nb, ng, co, ci, long long p, da, z, long long z_bstride, z_coef, gamma, part, int nslots,
    #  x, long long x_bstride, x_coef, int x_relu, float *dz, dw, dgamma, dbeta, coef_ws, d_row_bias,
    #  int rb_group, void *workspace, size_t workspace_bytes, int defer, void *stream)
    "nesie_pw_wgrad_bn_backward": (ctypes.c_int, "IIIIL" "PPL" "PPPI" "PLPI" "PPPPPP" "I" "PZ" "I" "P"),
    # (int nb, ng, channels, long long p, int group, pool_group, pmax, pmin, const uint8_t *amax,
    #  amin, coef, int relu, float *pooled, uint8_t *argmax, float *zstar, void *stream)
    "nesie_pw_pool_finish": (ctypes.c_int, "IIILII" "PPPPP" "I" "PPP" "P"),
    # (int channels, nslots, double count, part, z_coef, gamma, bnb, dgamma, dbeta, stream)
    "nesie_pw_bnb_coef": (ctypes.c_int, "IID" "PPPPPP" "P"),
    # (int b, k, t, c, cls, bbox, surface, side, iou_s, iou, quality, int detach_sigma,
    #  const long long *obj_t, label, obj_w, box_w, bbox_t, centre_t, valid_w, config, loss,
    #  s_cls, s_centre, s_surface, s_iou, s_iou_s, s_side_surf, s_side_iou, s_side_pred,
    #  sem_pick, kstar, dmin, partial, ticket, stream)
    "nesie_head_loss_forward_unsup": (ctypes.c_int, "IIII" "PPPPPPP" "I" "PPPPPPP" "PP" "PPPPPPPP"
                                      "PPPPP" "P"),
    # (int b, k, c, g, const long long *label, s_robj, s_angle, s_rot, s_sidej, d_robj, d_angle,
    #  d_rot, d_side, stream)
    "nesie_saqe_extra_loss_backward": (ctypes.c_int, "III" "PPPPPP" "PPPP" "P"),
    "nesie_fps_workspace_bytes": (ctypes.c_size_t, "II"),           # size_t (int b, int n)
    "nesie_mlp_stream_partials": (ctypes.c_longlong, "IL"),         # long long (int b, long long p)
    "nesie_last_error": (ctypes.c_char_p, ""),                      # const char * (void)
    "nesie_pw_wgrad_drop_deferred": (ctypes.c_int, ""),             # int (void)
}


def test_parser_agrees_with_prototypes_written_out_by_hand():
    assert len(HAND_WRITTEN["nesie_pw_layer_forward"][1]) == 26
    for name, (restype, codes) in HAND_WRITTEN.items():
        got_restype, got_argtypes = _lib.SIGNATURES[name]
        assert got_restype is restype, name
        assert got_argtypes == [_CODES[c] for c in codes], name


def test_parser_reads_every_spelling_the_headers_use():
    protos = _lib.parse_prototypes("""
        /* int nesie_in_a_comment(int a); */
        // size_t nesie_in_a_line_comment(void);
        #define NESIE_NOT_A_PROTOTYPE(x) nesie_macro(x)
        typedef enum { NESIE_OK = 0 } nesie_status;
        int nesie_all(int a, float b, double c, long long d, size_t e, const float *f,
                      const long long *g, uint8_t *h, const void *i,
                      void *stream);
        size_t nesie_bytes(void);
        long long nesie_count();
        const char *nesie_text(void);
    """)
    c = ctypes
    assert protos == {
        "nesie_all": (c.c_int, [c.c_int, c.c_float, c.c_double, c.c_longlong, c.c_size_t]
                      + [c.c_void_p] * 5),
        "nesie_bytes": (c.c_size_t, []),
        "nesie_count": (c.c_longlong, []),
        "nesie_text": (c.c_char_p, []),
    }


def test_parser_refuses_a_type_it_does_not_know():
    import pytest
    with pytest.raises(TypeError, match="nesie_narrow.*short n"):
        _lib.parse_prototypes("int nesie_ok(int a);\nint nesie_narrow(int a, short n, void *stream);")
    with pytest.raises(TypeError, match="nesie_wide.*unsigned long"):
        _lib.parse_prototypes("int nesie_wide(unsigned long n);")
    with pytest.raises(TypeError, match="nesie_ret.*unsigned"):
        _lib.parse_prototypes("unsigned nesie_ret(int a);")


def test_call_is_for_functions_that_return_a_status():
    import pytest
    for name in ("nesie_fps_workspace_bytes", "nesie_mlp_stream_partials", "nesie_last_error"):
        with pytest.raises(TypeError, match=name):
            _lib.call(name)


def test_launch_helper_refuses_a_call_the_header_does_not_describe(monkeypatch):
    """Every refusal comes before the library is reached (so none of this needs a GPU)."""
    import pytest
    import torch
    from nesie_amd import kernels

    def no_call(name, *args):
        raise AssertionError(f"{name} reached the library")
    monkeypatch.setattr(_lib, "call", no_call)
    x, i = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    # int nesie_gather_rows3(int b, int n, int m, const float *xyz, const int *sample, float *out,
    #                        void *stream)
    with pytest.raises(RuntimeError, match="need HIP device tensors.*no CPU path"):
        kernels._launch("nesie_gather_rows3", x, 1, 4, 4, x, i, x)
    with pytest.raises(TypeError, match="nesie_gather_rows3"):
        kernels._launch("nesie_gather_rows3", x, 1, 4, 4, x, i)          # one too few
    with pytest.raises(TypeError, match="nesie_gather_rows3"):
        kernels._launch("nesie_gather_rows3", x, 1, 4, 4, x, i, x, x)    # one too many
    with pytest.raises(TypeError, match="nesie_gather_rows3: argument 2 is a c_int"):
        kernels._launch("nesie_gather_rows3", x, 1, 4, i, x, i, x)       # a tensor for int m
    with pytest.raises(TypeError, match="nesie_gather_rows3: argument 3 is a pointer"):
        kernels._launch("nesie_gather_rows3", x, 1, 4, 4, 0.5, i, x)     # a float for xyz
    # int nesie_ball_query_wrapper(int b, int n, int m, float min_radius, float max_radius, ...)
    with pytest.raises(TypeError, match="nesie_ball_query_wrapper: argument 3 is a c_float"):
        kernels._launch("nesie_ball_query_wrapper", x, 1, 4, 4, None, 1.0, 2, x, x, i)


def test_invalid_arguments_return_a_status_not_a_crash():
    lib = _lib.load()
    # negative size -> NESIE_ERR_INVALID_ARG, no launch attempted (safe without a GPU)
    st = lib.nesie_ball_query_wrapper(-1, 4, 4, 0.0, 1.0, 2, None, None, None, None)
    assert st == 1
    assert b"ball_query_wrapper" in lib.nesie_last_error()
    # empty problems succeed without touching the device
    assert lib.nesie_group_points_forward(0, 3, 5, 2, 2, None, None, None, None) == 0
    assert lib.nesie_furthest_point_sampling_wrapper(2, 10, 0, None, None, None, None) == 0


def test_layer_entry_points_refuse_a_negative_batch_before_any_launch():
    """The layer kernels' entry points with nb = -1: status 1, the message names the entry point, and
    a call that asked for a deferred reduction has queued nothing.  The refusal comes before any HIP
    call (safe without a GPU)."""
    lib = _lib.load()
    assert lib.nesie_abi_version() == 2
    n = None
    calls = {
        "pw_layer_forward": lambda: lib.nesie_pw_layer_forward(
            -1, 1, 64, 64, 64, n, 0, n, 0, 64, 1, n, 1, n, 0, n, n, 0, n, 0, 0, n, n, n, n, n),
        "pw_wgrad": lambda: lib.nesie_pw_wgrad(-1, 1, 64, 64, 64, n, 0, n, 0, n, 1, n, n, 0, 1, n),
        "pw_wgrad_bn_backward": lambda: lib.nesie_pw_wgrad_bn_backward(
            -1, 1, 64, 64, 64, n, n, 0, n, n, n, 1, n, 0, n, 1, n, n, n, n, n, n, 0, n, 0, 1, n),
        "pw_pool_finish": lambda: lib.nesie_pw_pool_finish(-1, 1, 64, 64, 16, 16, n, n, n, n, n, 1, n, n, n, n),
    }
    for name, call in calls.items():
        assert call() == 1, name
        assert name.encode() in lib.nesie_last_error(), name
        assert lib.nesie_pw_wgrad_pending() == 0, name


def test_product_path_refuses_cpu_tensors():
    import pytest
    import torch
    from nesie_amd.mmdet3d_ops import ball_query, furthest_point_sample
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        furthest_point_sample(torch.rand(1, 32, 3), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ball_query(0.0, 0.5, 4, torch.rand(1, 32, 3), torch.rand(1, 4, 3))


def test_package_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "nesie_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), \
                    f"{f} imports the oracle"


def test_cu_budget_is_validated_and_restored():
    """nesie_set_cu_count: host-side sizing state only (no GPU call): multiples of 8 in [8, 256],
    anything else is refused with the usual status + message; HipKernels.cu_budget restores the
    previous value on exit, also when the body raises."""
    import pytest
    from nesie_amd.kernels import HipKernels
    lib = _lib.load()
    assert lib.nesie_get_cu_count() == 256
    for bad in (0, 4, 100, 260, -8):
        with pytest.raises(RuntimeError, match="set_cu_count"):
            _lib.call("nesie_set_cu_count", bad)
    assert lib.nesie_get_cu_count() == 256
    with HipKernels.cu_budget(232):
        assert lib.nesie_get_cu_count() == 232
        with HipKernels.cu_budget(248):
            assert lib.nesie_get_cu_count() == 248
        assert lib.nesie_get_cu_count() == 232
    assert lib.nesie_get_cu_count() == 256
    with pytest.raises(ValueError):
        with HipKernels.cu_budget(224):
            raise ValueError("body failed")
    assert lib.nesie_get_cu_count() == 256
