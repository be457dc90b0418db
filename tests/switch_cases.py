"""Registry of the WTPSE_ environment switches: every name the library reads with getenv() (csrc/) or the package with
os.environ.get() (wtpse_hip/) maps to what covers the code behind it — a job of tests/switch_worker.py (a child process started under
the variable: most are read once per process), a test id, or ("exempt", reason).  test_switch_paths_cpu.py fails on a name that is read
but not listed, and on a listed name that nothing reads any more.  profiles/switch_paths.md is the table in prose."""

_ROUTE = ("a route constant of nn.py: it chooses between entry points that each have kernel-level tests; a step-level matrix against "
          "the calibrated oracle bands is a separate piece of work")
_BUILD = "a build variable: it changes how the library is compiled, not what a kernel is asked to do"

SWITCHES = {
    # ---- csrc/: launch paths
    "WTPSE_X3_SMALL_WIDE":   "tests/test_exact_conv_gpu.py::test_conv_x3_small_wide",        # through its setter wtpse_x3_small_wide()
    "WTPSE_X3R":             "tests/test_exact_conv_gpu.py::test_conv_x3",                   # through its setter wtpse_x3r_enable(): tables x3r, x3half
    "WTPSE_X3_TERMS":        "tests/test_exact_conv_gpu.py::test_conv_x3",                   # through its setter wtpse_x3_terms(): every mode
    "WTPSE_X3_WGRAD_TW32":   ("job", "tw32"),
    "WTPSE_X3_MT":           ("job", "mt2", "mt1"),
    "WTPSE_X3_HALF_MIN":     ("job", "half1"),
    "WTPSE_TAIL_MAX_WGS":    ("job", "tail0"),
    "WTPSE_X3_HALF":         ("exempt", "=0 sends the x3half launches back to the 32-channel blocks: the same decision, and the same kernels, as "
                                        "wtpse_x3r_enable(0), under which test_conv_x3 runs the x3half table"),
    "WTPSE_X3_WGS":          ("exempt", "changes the split count of conv_wgrad_x3_k, which the WGX3 / tw32 tables already vary (1 ... 20 slabs)"),
    "WTPSE_WGRAD_R_WAVES":   ("exempt", "changes the slab count of wgrad_r_k, which the WGR table already varies (1 ... 220 slabs)"),
    "WTPSE_WGRAD_R_TWIN":    ("exempt", "=0 sends W = 16 to conv_wgrad_x3_k on 16-wide tiles, which the WGX3 table covers at W <= 24"),
    "WTPSE_C16_XCD":         "tests/test_conv_x3_gpu.py::test_xcd_order_equals_dispatch_order",
    "WTPSE_X3_XCD":          "tests/test_conv_x3_gpu.py::test_xcd_order_equals_dispatch_order",
    # ---- wtpse_hip/: build
    "WTPSE_EXTRA_HIPCC_FLAGS": ("exempt", _BUILD),
    "WTPSE_BUILD_JOBS":        ("exempt", _BUILD),
    "WTPSE_DEBUG":             ("exempt", "a host-side assertion on the ticket ring (ops._tickets): no kernel behind it"),
    # ---- wtpse_hip/nn.py: routes
    "WTPSE_X3":                    ("exempt", _ROUTE),
    "WTPSE_X3_FWD":                ("exempt", _ROUTE),
    "WTPSE_X3_DGRAD":              ("exempt", _ROUTE),
    "WTPSE_X3_WGRAD":              ("exempt", _ROUTE),
    "WTPSE_X16":                   ("exempt", _ROUTE),
    "WTPSE_X16_MIN_K":             ("exempt", _ROUTE),
    "WTPSE_WGRAD_R":               ("exempt", _ROUTE),
    "WTPSE_FWD_AMAX":              ("exempt", _ROUTE),
    "WTPSE_BN_FUSED_STATS":        ("exempt", _ROUTE),
    "WTPSE_BN_TAIL":               ("exempt", _ROUTE),
    "WTPSE_BN_IN":                 ("exempt", _ROUTE),
    "WTPSE_WT_FUSED_GRAM":         ("exempt", _ROUTE),
    "WTPSE_WGRAD_STREAM":          ("exempt", _ROUTE),
    "WTPSE_TEACHER_STREAM":        ("exempt", _ROUTE),
    "WTPSE_CONVU_REFERENCE_ORDER": ("exempt", _ROUTE),
}

# job -> (the one variable its child process is started under, its value, timeout in seconds).  The timeouts are five times the
# durations measured on an MI355X (profiles/switch_paths.md), interpreter start and a cold library load included in the measurement.
JOBS = {
    "tw32":  ("WTPSE_X3_WGRAD_TW32", "1", 15),
    "mt2":   ("WTPSE_X3_MT", "2", 20),
    "mt1":   ("WTPSE_X3_MT", "1", 35),
    "half1": ("WTPSE_X3_HALF_MIN", "1", 20),
    "tail0": ("WTPSE_TAIL_MAX_WGS", "0", 25),
}
