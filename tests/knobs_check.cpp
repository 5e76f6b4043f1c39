// Stand-alone host program around the library's knob table (tests/test_knobs.py compiles it with the system C++ compiler and runs it as a child
// process under a set environment): the header, its storage file, nothing else.
//   knobs_check dump                 every row as  name|kind|when|default|value|set|text
//   knobs_check reload NAME VALUE    the row before / after setenv(NAME, VALUE) without a reload / read live / after bofi_reload_env
#include <cstdio>
#include <cstring>

#include "bofi_knobs.h"
#include "knobs.hip"

static int find(const char* name) {
    for (int k = 0; k < bofi::KNOB_COUNT; ++k)
        if (!strcmp(bofi::g_knob_rows[k].name, name)) return k;
    return -1;
}

static void show(const char* tag, const bofi::KnobValue& v) { printf("%s %d %d %s\n", tag, v.i, (int)v.set, v.s ? v.s : "-"); }

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "dump")) {
        static const char* kinds[] = {"INT", "INTP", "STR"};
        static const char* whens[] = {"RELOAD", "CREATE"};
        for (int k = 0; k < bofi::KNOB_COUNT; ++k) {
            const bofi::KnobRow& r = bofi::g_knob_rows[k];
            const bofi::Knob id = (bofi::Knob)k;
            printf("%s|%s|%s|%d|%d|%d|%s\n", r.name, kinds[r.kind], whens[r.when], r.dflt, bofi::knob(id), (int)bofi::knob_set(id), bofi::knob_str(id) ? bofi::knob_str(id) : "-");
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "reload")) {
        const int k = find(argv[2]);
        if (k < 0) return 2;
        const bofi::Knob id = (bofi::Knob)k;
        const int gen0 = bofi::g_env_generation;
        show("first", bofi::knob_value(id));
        setenv(argv[2], argv[3], 1);
        show("stale", bofi::knob_value(id));
        show("live", bofi::knob_live(id));
        bofi_reload_env();
        show("reloaded", bofi::knob_value(id));
        unsetenv(argv[2]);
        bofi_reload_env();
        show("unset", bofi::knob_value(id));
        printf("generations %d\n", bofi::g_env_generation - gen0);
        return 0;
    }
    return 2;
}
