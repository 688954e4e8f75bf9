// p2p_limits.hpp -- the two sizes of the direct exchange that host-only code needs as well (exchange_state.hpp; the
// kernels and the inbox layout are in p2p_exchange.hpp, which includes this).  No HIP.
#pragma once

namespace cdk {

constexpr int kP2PMaxRanks = 8;
constexpr int kP2PMaxCount = 2688;                 // >= the widest block record (2625 doubles)

}  // namespace cdk
