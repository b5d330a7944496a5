// stream_set.h -- what every device-resident stream set holds around its planner, beside the slot table
// (stream_slots.h): two pinned host tables used in turn, each with the event of its last copy to the device, and the
// event behind the set's last call.  One rotation per set: every call that fills a table (a push, Haitsma's blocks,
// Wang's and Panako's windows) takes the next one.  Which locks a call takes, whether it waits on the context's audio event and
// where its table lands on the device stay with the planner that owns the call.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "stream_slots.h"

namespace ucfp {
namespace streams {

struct Tables {
    uint8_t* tab_h[2] = {nullptr, nullptr};   // pinned tables, used in turn
    hipEvent_t tab_copied[2] = {nullptr, nullptr};
    int tab_next = 0;
    hipEvent_t done = nullptr;            // behind the set's last call: the next one waits for it

    // on failure the caller tears down what exists
    hipError_t setup(size_t tab_bytes) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipHostMalloc((void**)&tab_h[i], tab_bytes, 0);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&tab_copied[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        return e;
    }

    // waits for the set's last call first: the owner frees its device state after this
    void teardown() {
        if (done) (void)hipEventSynchronize(done);
        for (int i = 0; i < 2; i++) {
            if (tab_h[i]) (void)hipHostFree(tab_h[i]);
            if (tab_copied[i]) (void)hipEventDestroy(tab_copied[i]);
        }
        if (done) (void)hipEventDestroy(done);
    }

    // the next pinned table; the one it replaces was copied two calls ago.  The caller fills tab_h[*k], enqueues its
    // copy and records tab_copied[*k] behind it.
    int next(int* k) {
        *k = tab_next;
        tab_next ^= 1;
        HIP_TRY(hipEventSynchronize(tab_copied[*k]));
        return UCFP_OK;
    }
};

}  // namespace streams
}  // namespace ucfp
