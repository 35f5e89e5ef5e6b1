// error.h -- the one declaration of the library's error setter (defined in genphi_hip.hip): stores the text genphi_last_error returns
// for the calling thread and hands `code` back, so that a failure reads `return genphi_set_error(code, text);`.  No HIP here: the host-only
// units include it, and the stand-alone test programs that build them define a stub of their own.
#pragma once
#include <string>

int genphi_set_error(int code, const std::string &msg);
