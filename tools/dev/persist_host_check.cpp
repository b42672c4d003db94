// Stand-alone check of the host half of csrc/persist.hpp, meant for a sanitizer build on a machine without a GPU (tools/dev/README.md):
// persistent_grid, the profiling-event guard on the normal and the early-return path, and a trace scope that is switched off.
// Nothing here touches a device.
#include "../../soccernet-calibration-sportlight_amd/csrc/persist.hpp"
#include <cstdio>
#include <string>

namespace sncal { int release_solve_scratch(hipStream_t, bool) { return 0; } }      // (api.cpp's only reference into the kernels' units)

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static int helper_that_fails() {
    sncal::LaunchEventsHold hold;
    CHECK(!sncal::launch_events().start && !sncal::launch_events().stop);
    return SNCAL_ERR_HIP;                                // the early return of run_tt / run_bblockx3 when a helper launch fails
}

int main() {
    using namespace sncal;
    CHECK(persistent_grid(256) == 256 && persistent_grid(304) == 304 && persistent_grid(100) == 96 && persistent_grid(8) == 8);
    CHECK(persistent_grid(7) == 256 && persistent_grid(0) == 256 && persistent_grid(-1) == 256);
    int a = 0, b = 0;                                    // stand-ins for two events: the guard only moves the handles
    const hipEvent_t e0 = reinterpret_cast<hipEvent_t>(&a), e1 = reinterpret_cast<hipEvent_t>(&b);
    launch_events().start = e0; launch_events().stop = e1;
    {
        LaunchEventsHold hold;
        CHECK(!launch_events().start && !launch_events().stop && hold.armed.start == e0 && hold.armed.stop == e1);
    }
    CHECK(launch_events().start == e0 && launch_events().stop == e1);
    CHECK(helper_that_fails() == SNCAL_ERR_HIP);
    CHECK(launch_events().start == e0 && launch_events().stop == e1);
    launch_events() = LaunchEvents{};
    {
        TraceScope off(nullptr, 1024, nullptr);          // no dump file: nothing allocated, nothing written
        CHECK(off.words == nullptr);
    }
    set_error("%s %d", "text", 7);
    CHECK(std::string(sncal_last_error()) == "text 7");
    printf(fails ? "persist_host_check: %d FAILED\n" : "persist_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
