// PathTracerState.h — the reference's PathTracerState (PathTracerMain.cpp:71-93; the OptiX handles collapse into one context),
// in a header of its own so that the query commands (QueryCommands.h) take the same state as the functions of PathTracerMain.cpp.
#pragma once
#include "../../include/acgpt.h"
#include "DeviceBuffer.h"

struct PathTracerState {
    pt_ctx* context = nullptr;
    pt_params params = {};
    acgpt::DeviceBuffer accumulation;                   // owns params.accumulationBuffer
    int device = 0;
    int gpus = 1;                                       // > 1: one context over devices 0..gpus-1
    bool multi = false;                                 // --multi: the group context even for one device (its RCCL reduce then runs with one rank)
};
