// Translation unit of the row-chain kernels with the out-proj -> GLU head, encoder_dim 256 (rowchain.hip.h).
#include "rowchain.hip.h"

hipError_t launch_rowchain_256_head(hipStream_t s, const ChainArgs &a, bool taps, int rows_hint) { return launch_rowchain_head<256>(s, a, taps, rows_hint); }
