// api_guard.h -- the extern "C" error boundary (include/qasr.h), stated once for every handle kind: exceptions never cross it.
// Host C++ only.  A handle type H takes part by declaring, before its first use here,
//     std::string& error_slot(const H* h);      // the handle's message slot, create_error<Tag>() for a null handle
#pragma once
#include "common.h"
#include "qasr.h"
#include <cstring>
#include <string>

// What qasr_*_last_error(NULL) answers after a failed create: one thread-local slot per tag, shared by every file that names the tag.
template <class Tag> std::string& create_error() {
    static thread_local std::string slot;
    return slot;
}

template <class H> int fail(const H* h, int code, const std::string& msg) {
    // a reported HIP failure must not stay behind as the runtime's sticky "last error" (a later launch check would blame itself for it)
    if (code == QASR_ERR_HIP) (void)hipGetLastError();
    error_slot(h) = msg;
    return code;
}

// Runs f(); what it throws becomes a status, with the message in the handle's slot.
template <class H, class F> int guarded(const H* h, F&& f) {
    try { f(); return QASR_OK; }
    catch (const qasr::HipError& ex) { return fail(h, QASR_ERR_HIP, ex.what()); }
    catch (const qasr::NotLoaded& ex) { return fail(h, QASR_ERR_NOT_LOADED, ex.what()); }
    catch (const std::invalid_argument& ex) { return fail(h, QASR_ERR_INVALID, ex.what()); }
    catch (const std::length_error& ex) { return fail(h, QASR_ERR_CAPACITY, ex.what()); }
    catch (const std::exception& ex) { return fail(h, QASR_ERR_INVALID, ex.what()); }
}

// The create sequence: a fresh handle, init(handle); on a throw the handle is deleted, the message goes to the create-error slot and the
// status is QASR_ERR_HIP for a HIP failure, `other` for anything else.
template <class H, class F> int guarded_create(H** out, int other, F&& init) {
    H* h = new H();
    try { init(h); }
    catch (const qasr::HipError& ex) { delete h; return fail<H>(nullptr, QASR_ERR_HIP, ex.what()); }
    catch (const std::exception& ex) { delete h; return fail<H>(nullptr, other, ex.what()); }
    *out = h;
    return QASR_OK;
}

// t with its terminator into the caller's buffer: its length, or -1 when cap is too small
inline int copy_out(const std::string& t, char* buf, size_t cap) {
    if (t.size() + 1 > cap) return -1;
    std::memcpy(buf, t.c_str(), t.size() + 1);
    return (int)t.size();
}
