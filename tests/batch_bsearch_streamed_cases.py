"""The cases of tests/test_gpu_batch_bsearch_streamed.py, apart from the tests so that tests/test_batch_bsearch_streamed_cpu.py
can assert on the reference records (tests/batch_bsearch_reference.py) what each case is there to cover.  Test
infrastructure, not product code.

With the stock interval (-50, 50) every probe of the seeded family at n >= 64 is feasible at once, so the cases past one wave
take intervals that straddle the optimum: their probes end feasible, by a failed cut and by inner_max_iters, some feasible
probe comes after two cuts or more, and a member makes five oracle calls per probe or more."""
import batch_bsearch_reference as ref

WIDE, SHORT = (2000, 1e-8), (25, 1e-8)


class Case:
    def __init__(self, n, B, interval, inner, outer, straddles=True, max_end=True):
        self.n, self.B, self.interval, self.inner, self.outer = n, B, interval, inner, outer
        self.straddles = straddles  # the coverage conditions hold (asserted by the CPU test)
        self.max_end = max_end      # ... a probe that ends by inner_max_iters among them
        self.id = f"n{n}-B{B}-lo{interval[0]:g}-inner{inner[0]}-tol{inner[1]:g}"

    def want(self, stable, B=None, **kw):
        return ref.runs(self.n, self.B if B is None else B, stable, self.inner, self.outer, interval=self.interval, **kw)


STOCK = ref.INTERVAL
N129 = Case(129, 4, (-400.0, 0.0), (40, 1e-8), (10, 1e-8))
FAMILY = [
    Case(2, 9, STOCK, WIDE, ref.OUTER, straddles=False),
    Case(2, 9, STOCK, SHORT, ref.OUTER, straddles=False),
    Case(5, 6, STOCK, SHORT, ref.OUTER, straddles=False),
    Case(65, 3, STOCK, (30, 1e-8), (6, 1e-8), straddles=False),
    Case(65, 3, (-200.0, 0.0), (40, 1e-8), (10, 1e-8)),
    Case(128, 2, (-400.0, 0.0), (40, 1e-8), (10, 1e-8)),
    N129,
    Case(129, 4, (-400.0, 0.0), (40, 150.0), (10, 1e-8), straddles=False),  # the route to an end by the tolerance
    Case(130, 3, (-400.0, 0.0), (25, 1e-8), (10, 1e-8)),
    Case(193, 4, (-500.0, 0.0), (40, 1e-8), (10, 1e-8)),
    Case(256, 3, (-600.0, 0.0), (40, 1e-8), (8, 1e-8)),
    Case(1024, 2, (-3000.0, 0.0), (10, 1e-8), (5, 1e-8), max_end=False),
]
TOL_END = FAMILY[7]


class CountingLinFeas(ref.LinFeas):
    """LinFeas that keeps, per probe (update call), the number of oracle calls and whether the last one was feasible"""

    def __init__(self, a, c):
        super().__init__(a, c)
        self.probes = []

    def update(self, gamma):
        super().update(gamma)
        self.probes.append([0, False])

    def assess_feas(self, x):
        cut = super().assess_feas(x)
        self.probes[-1][0] += 1
        self.probes[-1][1] = cut is None
        return cut


def probes_of(case, seed, stable):
    """[(oracle calls, ended feasible)] of every probe of member `seed`"""
    a, c, xc0 = ref.family(seed, case.n)
    omega, space = CountingLinFeas(a, c), ref.space_of(stable, xc0)
    ref.bsearch(omega, space, case.interval[0], case.interval[1], case.inner, case.outer)
    return [tuple(p) for p in omega.probes]
