// Test infrastructure, not product code: what the stand-alone host-check drivers (tests/hostcheck_*/) share.
#pragma once

#include <stdio.h>
#include <stdlib.h>

// every heap block of a run, freed when main returns on whichever path (a refusal included): the sanitizer build counts leaks
struct Blocks {
    void* p[64];
    int n = 0;
    void* keep(void* q) {
        if (!q || n >= 64) exit(1);
        return p[n++] = q;
    }
    ~Blocks() {
        for (int i = 0; i < n; ++i) free(p[i]);
    }
};

// the next `bytes` of a request file in a block of its own (`owner`'s, when given); a short file ends the run with code 1
static inline void* read_block(FILE* f, size_t bytes, Blocks* owner = nullptr) {
    void* p = malloc(bytes ? bytes : 1);
    if (owner) owner->keep(p);
    if (!p || fread(p, 1, bytes, f) != bytes) exit(1);
    return p;
}
