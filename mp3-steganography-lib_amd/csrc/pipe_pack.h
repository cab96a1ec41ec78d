// The packed area of a slot's stage: a job's parts one after the other, each on a 16-byte boundary, so that one copy takes them up.  A preparer
// states its parts in their order (the four layouts: DESIGN.md 3.1a); the arithmetic and the ONE capacity check are here.
#pragma once
#include <stddef.h>

struct StagePacker {
    size_t at = 0, bound = 0;
    bool ok = true;                                        // every part so far ended at or in front of `bound`
    static size_t align(size_t x) { return (x + 15) & ~(size_t)15; }
    void begin(size_t start, size_t limit) { at = start; bound = limit; ok = start <= limit; }
    size_t add(size_t bytes) { const size_t o = align(at); ok = ok && o <= bound && bytes <= bound - o; at = o + bytes; return o; }   // a part: its offset
    size_t end() const { return at; }
};
