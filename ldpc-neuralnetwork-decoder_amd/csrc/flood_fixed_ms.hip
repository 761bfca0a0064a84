// flood_fixed_ms.hip -- flood_fixed_kernel instances for scaled min-sum (compile-time schedules of the reference's codes).
// Split out of flood.hip so that the kernel families compile in parallel.
#include "flood_fixed.hpp"

namespace ldpc {

template int launch_fixed<LDPC_ALGO_MINSUM>(const FloodCall &, int, size_t, const Outs &, const EsWs &, uint32_t *);

}  // namespace ldpc
