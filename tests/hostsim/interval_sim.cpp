// interval_sim.cpp — the host arithmetic of the interval route (csrc/tsq_dapack.h: tsq_da_is_interval, tsq_da_outside) behind a C
// interface, for tests/test_interval_plan_cpu.py (which compiles this file on its own: it is not part of hostsim.so).
#include <cstdint>

#include "../../tinysql_amd/csrc/tsq_dapack.h"

extern "C" {
int sim_da_is_interval(uint64_t usable, uint64_t range, int unique) { return tsq_da_is_interval(usable, range, unique != 0) ? 1 : 0; }
// 1: a probe cell k cannot match a build side with the domain [kmin, kmin + range] (skip_high: the columns differ in signedness)
int sim_da_outside(uint64_t kmin, uint64_t range, int skip_high, uint64_t k) {
    DaDomain dm{kmin, range, 0, 0, 0, skip_high};
    return tsq_da_outside(dm, k) ? 1 : 0;
}
// the plan of a build side and its verdict in one call, as da_prepare takes them: kmin / kmax in the join's order, byte cells only
int sim_da_plan_interval(uint64_t kmin, uint64_t kmax, uint64_t usable, int skip_high, int unique) {
    const DaPlan pl = tsq_da_plan(kmin, kmax, usable, skip_high, true, true);
    if (!pl.ok) return -1;
    return (!pl.bit_cells && tsq_da_is_interval(usable, pl.dm.range, unique != 0)) ? 1 : 0;
}
}
