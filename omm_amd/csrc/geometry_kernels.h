// geometry_kernels.h -- triangles from a micromap (geometry_kernels.hip): the cut of a device-resident result into opacity-sorted nodes of the bird
// curve (ommxExtractMicroGeometry; omm_host.cpp owns the baker, its device pool and the argument checks) and the vertices of such nodes
// (ommxExpandMicroNodes, defined in geometry_kernels.hip like ommxLookupOpacity in lookup_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/omm_mi355x_ext.h"

namespace ommx {

struct GeoArgs {
    ommCpuBakeResultDesc result;   // host struct, arrays in device memory; indexFormat already checked, indexCount > 0
    uint8_t cls[4];                // class of ommOpacityState s: output list 0..3, or kGeoDrop
    uint8_t mixed;                 // class of a node at the emit level whose micro-triangles differ
    uint32_t emitLevel;            // min(maxEmitLevel, 12)
};

// The call is two halves with a host decision between them.  geo_count leaves every count and offset in the scratch block `head`
// (geo_head_bytes) and a per-tile block (`tiles`, geo_tile_bytes of the tile count that geo_count_tiles reports) and returns the totals;
// geo_emit writes the caller's arrays from them.  Every launch is on `stream`; both synchronise it.
struct GeoTotals { unsigned long long counts[4], primTiles; uint32_t skipped, pad; };
size_t geo_head_bytes(const GeoArgs& a);
hipError_t geo_count_tiles(const GeoArgs& a, void* head, unsigned long long* tileCount, hipStream_t stream);
size_t geo_tile_bytes(unsigned long long tileCount);
hipError_t geo_count(const GeoArgs& a, void* head, void* tiles, unsigned long long tileCount, bool wantEmit, GeoTotals* out, hipStream_t stream);
hipError_t geo_emit(const GeoArgs& a, const void* head, const void* tiles, unsigned long long tileCount, const GeoTotals& totals, const ommxMicroGeometryOutputs& o, hipStream_t stream);

} // namespace ommx
