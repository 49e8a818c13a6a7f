// QueryCommands.h — the query options of acgpt_main (--pick ... --cast-mesh) as one table, in the order they run.  main() looks an
// option up with findQueryCommand, hands its value to parse, asks check once the image size is known, and after "Launch
// Initialized" calls run on every entry that was given.  A new query option is one entry here (QueryCommands.cpp) and nothing in
// main(): DESIGN.md, "Where a query option of acgpt_main goes".
#pragma once
#include <string>
#include <vector>
#include "PathTracerState.h"
#include "TinyObjWrapper.h"

struct QueryCommand {
    const char* option;                                     // "--sweep"
    const char* usage;                                      // the line a refused value prints, with exit status 2
    bool (*parse)(const char* text);                        // appends one argument to the entry's own list, or returns false
    std::string (*check)(int width, int height);            // optional: "" or why an argument does not fit the image
    void (*run)(PathTracerState&, const acgpt::TinyObjWrapper&);   // one library call per batch, then one JSON line per argument
    size_t given;                                           // arguments parsed so far
};

std::vector<QueryCommand>& queryCommands();
QueryCommand* findQueryCommand(const std::string& option);
