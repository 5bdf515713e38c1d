// knob.h -- the only place liblrcn_hip reads the environment.  Every LRCN_* variable is looked up when the code that asks runs (never
// cached in a static): the tests flip them inside one process.  DESIGN.md "Environment variables" lists every name read through these.
#pragma once
#include <cstdlib>

inline bool knob_set(const char *name) { return getenv(name) != nullptr; }
// first character of the value; 0 when the variable is unset or empty
inline char knob_char(const char *name) {
    const char *v = getenv(name);
    return v ? v[0] : '\0';
}
inline bool knob_off(const char *name) { return knob_char(name) == '0'; }  // NAME=0 turns a default route off
inline int knob_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}
