// stream_slots.h -- the slot table of a device-resident stream set: which slots are open, how many units (samples or
// bytes) each has seen, and the per-call check that a slot is in range, open and named once.  Plain host C++ with no HIP
// in it (tests/native/stream_slots_check.cpp drives it on a CPU); stream_set.h adds the pinned tables and the events.
// Shared by the four kinds of set: Wang (A9), Panako (A19), Haitsma (A18) and MinHash text (T7).
//
// Every operation expects the set's mutex `mu` to be held.  `seen` is all zero whenever no call is in progress: a caller
// that marked entries un-marks its whole list before it returns, whether the call was accepted or refused.
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/ucfp_hip.h"

namespace ucfp {

int capi_fail(int code, const char* fmt, ...);   // capi.hip: sets the thread's last error message and returns `code`

namespace streams {

struct Slots {
    uint32_t max_streams = 0;
    std::mutex mu;                        // serialises the set's calls
    std::vector<uint64_t> n;              // units seen per slot
    std::vector<uint8_t> open;
    std::vector<uint8_t> seen;            // duplicate-slot check of one call

    void init(uint32_t slots) {
        max_streams = slots;
        n.assign(slots, 0);
        open.assign(slots, 0);
        seen.assign(slots, 0);
    }

    // the lowest free slot, opened with nothing seen
    int acquire(uint32_t* slot) {
        for (uint32_t i = 0; i < max_streams; i++) {
            if (!open[i]) {
                open[i] = 1;
                n[i] = 0;
                *slot = i;
                return UCFP_OK;
            }
        }
        return capi_fail(UCFP_E_INVALID, "all %u slots are open", max_streams);
    }

    int release(uint32_t slot) {
        if (slot >= max_streams || !open[slot]) return capi_fail(UCFP_E_INVALID, "slot %u is not open", slot);
        open[slot] = 0;
        n[slot] = 0;
        return UCFP_OK;
    }

    // a call names at most one entry per slot; `items` ("entries"), `what` ("call" or "push"): the caller's wording
    int fits(size_t count, const char* items, const char* what) const {
        if (count <= max_streams) return UCFP_OK;
        return capi_fail(UCFP_E_INVALID, "%zu %s in one %s, the set has %u slots", count, items, what, max_streams);
    }

    // one entry of a call: in range, open, not named before in this call; then marked
    int mark(uint32_t slot, const char* what) {
        if (slot >= max_streams) return capi_fail(UCFP_E_INVALID, "slot %u out of range [0, %u)", slot, max_streams);
        if (!open[slot]) return capi_fail(UCFP_E_INVALID, "slot %u is not open", slot);
        if (seen[slot]) return capi_fail(UCFP_E_INVALID, "slot %u appears twice in one %s", slot, what);
        seen[slot] = 1;
        return UCFP_OK;
    }

    // clears the marks of a list, whichever of its entries were marked (slots out of range never were)
    void unmark(const uint32_t* slots, size_t count) {
        for (size_t i = 0; i < count; i++)
            if (slots[i] < max_streams) seen[slots[i]] = 0;
    }

    // the whole list at once, for callers that judge every slot before anything else; nothing stays marked
    int check(const uint32_t* slots, size_t count, const char* items, const char* what) {
        int rc = fits(count, items, what);
        if (rc) return rc;
        for (size_t i = 0; i < count && rc == UCFP_OK; i++) rc = mark(slots[i], what);
        unmark(slots, count);
        return rc;
    }
};

}  // namespace streams
}  // namespace ucfp
