"""Which line lengths the per-stage tests of the general-length spectral path (csrc/resfft_gen.hip) run, chosen from the
library's own plans (mtd_spectral_gen_plan), so that a change of the planner changes the list with it.  Shared by the GPU
test (tests/test_spectral_gen_stages_gpu.py) and the CPU test that proves the list leaves no plan out
(tests/test_any_size_plan_cpu.py)."""
import ctypes

N_MIN, N_MAX = 16, 512
MODEL_SIDES = (77, 509)          # the Bluestein sides of the model-level tests (tests/test_any_size_gpu.py)


def library_plans(L):
    """{n: (M, radices)} for every length the path takes: M = 0 for a mixed-radix plan, else the Bluestein convolution
    length.  L is the caller's handle of the library (the GPU tests' hip_lib, a CPU test's own ctypes.CDLL): nothing here
    loads or builds it, so the first load of a GPU run stays behind the hip_lib fixture's build."""
    plans = {}
    for n in range(N_MIN, N_MAX + 1):
        out = (ctypes.c_int * 16)()
        k = L.mtd_spectral_gen_plan(n, out)
        assert k > 0, n
        plans[n] = (out[0], tuple(out[1:1 + k]))
    return plans


def select(plans):
    """(smooth, blue): every mixed-radix length, and per Bluestein M the smallest and the largest length that map to it, the
    smallest and the largest even one (an odd W has no Nyquist column), and the model-level sides."""
    smooth = [n for n in sorted(plans) if plans[n][0] == 0]
    by_m = {}
    for n in sorted(plans):
        if plans[n][0]:
            by_m.setdefault(plans[n][0], []).append(n)
    blue = {}
    for m, ns in sorted(by_m.items()):
        even = [n for n in ns if n % 2 == 0]
        pick = {ns[0], ns[-1]} | set(even[:1]) | set(even[-1:]) | {n for n in MODEL_SIDES if n in ns}
        blue[m] = sorted(pick)
    return smooth, blue
