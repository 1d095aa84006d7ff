// dab/tx/dabgpu_tx_check.h -- what the classes of dab/tx do with a status of libdabgpu.so: an exception that names the class
#pragma once
#include <stdexcept>
#include <string>

#include "dabgpu.h"

// "<Class>: <what>: <status> -- <the library's last error>"
inline void dabgpu_tx_check(const char* cls, int st, const char* what) {
    if (st != DABGPU_OK) throw std::runtime_error(std::string(cls) + ": " + what + ": " + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
}

// first thing in a constructor: the library loaded is the one this class was built for
inline void dabgpu_tx_check_abi(const char* cls) {
    if (dabgpu_abi_version() != DABGPU_ABI_VERSION)
        throw std::runtime_error(std::string(cls) + ": libdabgpu.so implements ABI version " + std::to_string(dabgpu_abi_version()) +
                                 ", this class was built for " + std::to_string(DABGPU_ABI_VERSION));
}
