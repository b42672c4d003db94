// Stand-alone check of csrc/env.hpp (the table of SNCAL_* switches and its accessors in api.cpp), meant for a sanitizer build on a machine
// without a GPU (tools/dev/README.md): defaults, the parsing of each kind, and which lifetimes follow a change of the variable.
// Nothing here touches a device.  A PROCESS row keeps its first value for the rest of the process, so every such row is read once only.
#include "../../soccernet-calibration-sportlight_amd/csrc/common.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

namespace sncal { int release_solve_scratch(hipStream_t, bool) { return 0; } }      // (api.cpp's only reference into the kernels' units)

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    using namespace sncal;
#define UNSET(id, name, kind, dflt, life, what) unsetenv(name);
    SNCAL_ENV_TABLE(UNSET)
#undef UNSET
    // unset: the row's default, on the rows that are read on every call
    CHECK(env_flag(ENV_CONV_TT) && env_flag(ENV_GROUP_CONVS) && env_int(ENV_FUSE_BNECK) == 3 && env_int(ENV_SUBBATCH) == 64);
    CHECK(env_int(ENV_TT_SMALL_ITEMS) == 2 && env_int(ENV_BBX_MAX_BYTES) == 0xf0000000ll);
    // FLAG: "0" is off, anything else on -- the empty string and "no" included; a NET row follows the variable
    const struct { const char* text; bool on; } flags[] = {{"", true}, {"0", false}, {"1", true}, {"no", true}};
    for (const auto& f : flags) {
        setenv("SNCAL_FUSED_HEAD", f.text, 1);
        CHECK(env_flag(ENV_FUSED_HEAD) == f.on);
    }
    unsetenv("SNCAL_FUSED_HEAD");
    CHECK(env_flag(ENV_FUSED_HEAD));
    // INT, on a LAUNCH row that follows the variable; values past 32 bits pass
    setenv("SNCAL_BBX_MAX_BYTES", "4700000", 1);
    CHECK(env_int(ENV_BBX_MAX_BYTES) == 4700000);
    setenv("SNCAL_BBX_MAX_BYTES", "6000000000", 1);
    CHECK(env_int(ENV_BBX_MAX_BYTES) == 6000000000ll);
    setenv("SNCAL_BBX_MAX_BYTES", "-3", 1);
    CHECK(env_int(ENV_BBX_MAX_BYTES) == -3);
    setenv("SNCAL_BBX_MAX_BYTES", "junk", 1);
    CHECK(env_int(ENV_BBX_MAX_BYTES) == 0);
    unsetenv("SNCAL_BBX_MAX_BYTES");
    CHECK(env_int(ENV_BBX_MAX_BYTES) == 0xf0000000ll);
    // PROCESS rows: the default when unset at the first read, kept when the variable appears afterwards
    CHECK(!env_flag(ENV_PROFILE_DETAIL) && env_int(ENV_HEAD32) == 1 && env_str(ENV_BB_TRACE) == nullptr);
    setenv("SNCAL_PROFILE_DETAIL", "1", 1); setenv("SNCAL_HEAD32", "0", 1); setenv("SNCAL_BB_TRACE", "late.bin", 1);
    CHECK(!env_flag(ENV_PROFILE_DETAIL) && env_int(ENV_HEAD32) == 1 && env_str(ENV_BB_TRACE) == nullptr);
    // ... and the first value kept after the variable changes or goes: STR passes the text through, as the accessor's own copy
    setenv("SNCAL_TT_TRACE", "first.bin", 1);
    CHECK(env_str(ENV_TT_TRACE) && std::string(env_str(ENV_TT_TRACE)) == "first.bin");
    setenv("SNCAL_TT_TRACE", "second.bin", 1);
    CHECK(std::string(env_str(ENV_TT_TRACE)) == "first.bin");
    unsetenv("SNCAL_TT_TRACE");
    CHECK(std::string(env_str(ENV_TT_TRACE)) == "first.bin");
    setenv("SNCAL_SOLVE_TASKS", "0", 1);
    CHECK(!env_flag(ENV_SOLVE_TASKS));
    setenv("SNCAL_SOLVE_TASKS", "1", 1);
    CHECK(!env_flag(ENV_SOLVE_TASKS));
    // every PROCESS row caches on its OWN first read: B, set after A was read, is still seen
    setenv("SNCAL_HEADX3", "0", 1);
    CHECK(env_int(ENV_HEADX3) == 0);
    setenv("SNCAL_HEAD_STAGE", "0", 1);
    CHECK(env_int(ENV_HEAD_STAGE) == 0);
    setenv("SNCAL_TT_TRACE_CFG64", "1", 1);                       // (a FLAG whose default is off)
    CHECK(env_flag(ENV_TT_TRACE_CFG64));
    setenv("SNCAL_SOLVE_WAVE_WGS", "0", 1);
    CHECK(!env_flag(ENV_SOLVE_WAVE_WGS));
    setenv("SNCAL_SOLVE_SCHEDULE", "converged", 1);
    CHECK(std::string(env_str(ENV_SOLVE_SCHEDULE)) == "converged");
    printf(fails ? "env_host_check: %d FAILED\n" : "env_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
