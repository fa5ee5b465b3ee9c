// rebuild_arrays.h -- the arrays an operation hands to the tail of a derived result (rebuild_kernels.h), laid out once for ommxCoarsenMicromap,
// ommxCombineMicromaps and ommxGatherMicromaps.  Plain C++ (no HIP), in bake_host.h's style: from a null base the cursor gives the bytes to reserve,
// from the scratch's base the pointers.  tests/native/rebuild_arrays_check.cpp runs it under sanitizers.
#pragma once
#include "bake_host.h"   // CarveCursor, pad256

namespace ommx {

struct TailArrays {
    uint32_t* item;                                  // [n] the words of rebuild_kernels.h
    unsigned long long *slotStart, *units;           // [n + 1] each: sizes, then (scanned in place) offsets of the staging slots and of the work units
    unsigned long long* digest; uint32_t* umask;     // [n] each
    uint8_t *temp, *tailScratch;                     // the scans' temporary storage; the tail's own scratch (rebuild_bytes)
    size_t tempBytes;
    size_t bytes;                                    // what these slots took of the cursor
};
// An operation carves its own arrays with the same cursor, before or after this.
inline TailArrays carve_tail_arrays(CarveCursor& c, size_t items, size_t tempBytes, size_t tailBytes)
{
    TailArrays t; const uintptr_t from = c.at;
    t.item = c.take<uint32_t>(items);
    t.slotStart = c.take<unsigned long long>(items + 1); t.units = c.take<unsigned long long>(items + 1);
    t.digest = c.take<unsigned long long>(items); t.umask = c.take<uint32_t>(items);
    t.temp = c.take<uint8_t>(tempBytes); t.tempBytes = tempBytes;
    t.tailScratch = c.take<uint8_t>(tailBytes);
    t.bytes = (size_t)(c.at - from);
    return t;
}

} // namespace ommx
