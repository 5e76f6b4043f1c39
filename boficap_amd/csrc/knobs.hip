// Storage and reader of the knob table (bofi_knobs.h), the reload generation and bofi_reload_env.  Host code only, plain C++: the one
// place of the library that calls getenv.
#include <string>

#include "bofi_knobs.h"

namespace bofi {

int g_env_generation = 0;
bool g_knobs_loaded = false;

const KnobRow g_knob_rows[KNOB_COUNT] = {
#define BOFI_KNOB_ROW(name, kind, dflt, when, doc) {#name, KNOB_##kind, dflt, KNOB_##when, doc},
    BOFI_KNOBS(BOFI_KNOB_ROW)
#undef BOFI_KNOB_ROW
};
KnobValue g_knob_values[KNOB_COUNT];
static std::string g_knob_text[KNOB_COUNT];                // the table's own copies of the STR rows (getenv's pointer dies with the next setenv)

KnobValue knob_live(Knob k) {
    const KnobRow& r = g_knob_rows[k];
    const char* e = getenv(r.name);
    return KnobValue{e && r.kind != KNOB_STR ? atoi(e) : r.dflt, e != nullptr, e};
}

void knobs_load() {
    for (int k = 0; k < KNOB_COUNT; ++k) {
        KnobValue v = knob_live((Knob)k);
        if (v.s) { g_knob_text[k] = v.s; v.s = g_knob_text[k].c_str(); }
        g_knob_values[k] = v;
    }
    g_knobs_loaded = true;
}

}  // namespace bofi

extern "C" void bofi_reload_env(void) {
    bofi::knobs_load();
    ++bofi::g_env_generation;
}
