// glu_gather_object.hpp -- the Gather object behind glu::Gather (glu_gather.hip owns its life and its calls).  It owns no device
// memory: a call needs no scratch, so there is nothing to prepare and every call is allocation-free.  The plan of a call is
// gather_walk.hpp's gather_plan.
#pragma once

#include "gather_walk.hpp"
#include "glu_tile_host.hpp"

struct glu_gather_s
{
    // what the last call enqueued
    struct Last
    {
        uint32_t tiles = 0, kernels = 0;
    } last;
    void release() {}
};
