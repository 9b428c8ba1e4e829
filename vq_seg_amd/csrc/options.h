// The keys of vqseg_set_option: every module keeps one table of these records, and apply_option is the only code that
// looks a key up and stores a value.  (The key list for people: INTEGRATION.md, "Dispatch options".)
#pragma once
#include <stddef.h>
#include <string.h>

namespace vqseg {

enum OptKind {
    OPT_INT,            // stored as given
    OPT_FLAG,           // stored as value ? 1 : 0
    OPT_RANGE_KEEP,     // lo..hi; outside: nothing stored, the current value is still the answer
    OPT_RANGE_FAIL,     // lo..hi; outside: answered like an unknown key
    OPT_POW2_FAIL,      // a power of two in lo..hi; anything else: answered like an unknown key
};

struct Option {
    const char* key;
    int* slot;
    OptKind kind = OPT_INT;
    int lo = 0, hi = 0;
};

// the previous value of `key`, or -1: unknown key (or a value its kind refuses)
template <size_t N>
inline int apply_option(const Option (&table)[N], const char* key, int value) {
    for (const Option& o : table) {
        if (!key || strcmp(key, o.key)) continue;
        const bool inside = value >= o.lo && value <= o.hi;
        if (o.kind == OPT_RANGE_FAIL && !inside) return -1;
        if (o.kind == OPT_POW2_FAIL && (!inside || (value & (value - 1)))) return -1;
        const int prev = *o.slot;
        if (o.kind == OPT_FLAG) *o.slot = value ? 1 : 0;
        else if (o.kind != OPT_RANGE_KEEP || inside) *o.slot = value;
        return prev;
    }
    return -1;
}

}  // namespace vqseg
