// flood_fixed_bp.hip -- flood_fixed_kernel instances for sum-product (BP) (compile-time schedules of the reference's codes).
// Split out of flood.hip so that the kernel families compile in parallel.
// The BP instances run without register edges: flood_fixed.hpp reg_edges().
#include "flood_fixed.hpp"

namespace ldpc {

template int launch_fixed<LDPC_ALGO_BP>(const FloodCall &, int, size_t, const Outs &, const EsWs &, uint32_t *);

}  // namespace ldpc
