"""The launch plan's C structs (tests/native/plan_io.h plan_in / plan_out) as ctypes structures,
for the tests that reach rt_launch_plan.h through ph_plan, sh_plan or fu_plan.  A field left out
of a constructor call is 0, which is every later field's "as before" value."""
import ctypes


class PlanIn(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("flags", "kernel", "count", "fast_chunk", "spp", "pass_spp")] + \
               [("n_pixels", ctypes.c_longlong), ("ray_depth", ctypes.c_int), ("n_nodes", ctypes.c_int),
                ("spec_blocks", ctypes.c_longlong), ("variant_blocks", ctypes.c_longlong), ("subset_items", ctypes.c_longlong)] + \
               [(n, ctypes.c_int) for n in ("fast_accum", "fast_units", "moments")]


class PlanOut(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("err", "lane", "v_count", "v_fast", "v_lsplit", "v_spec", "v_chain")] + \
               [("sched", ctypes.c_ulonglong)] + \
               [(n, ctypes.c_int) for n in ("handoff", "ordered", "cs", "chunks")] + \
               [("n_items", ctypes.c_longlong), ("round_min", ctypes.c_int), ("stats_spp", ctypes.c_int)] + \
               [(n, ctypes.c_longlong) for n in ("blocks", "slots", "groups", "per", "blocks2", "waves2", "dealt", "per2")] + \
               [(n, ctypes.c_int) for n in ("spread2", "v_mom", "variant_index", "mode", "mode2")] + \
               [("msg", ctypes.c_char * 192)]
