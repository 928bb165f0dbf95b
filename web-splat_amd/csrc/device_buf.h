// device_buf.h -- the one owner of a device allocation.  Every object behind the C ABI holds its device memory as DeviceBuf
// members, so a handle's destructor IS its free list and an early return frees what the function allocated so far.  The
// destructor frees WITHOUT synchronising: whoever lets a buffer go while a launch may still read it synchronises first, in the
// caller ("Device memory").  Plain C++: the runtime is reached only through the two functions below, which
// ws_api.cpp defines over hipMalloc / hipFree and a CPU test (tests/test_frame_scratch.py) over malloc / free.
#pragma once

#include <stddef.h>

#include "websplat.h"

namespace ws {

int device_alloc(void** p, size_t bytes);  // WS_OK, or the code of the failure with ws_last_error set; *p is null then
void device_free(void* p);                 // p != nullptr

template <typename T>
class DeviceBuf {  // move-only
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DeviceBuf() { reset(); }

    // `count` elements (0 counts as 1), after freeing what the buffer holds: the peak is one block, not two
    int alloc(size_t count) {
        reset();
        if (count == 0) count = 1;
        void* p = nullptr;
        if (const int rc = device_alloc(&p, count * sizeof(T))) return rc;
        p_ = static_cast<T*>(p), n_ = count;
        return WS_OK;
    }
    void reset() {
        if (p_) device_free(p_);
        p_ = nullptr, n_ = 0;
    }
    T* get() const { return p_; }
    size_t count() const { return n_; }  // elements; 0 = empty
    size_t bytes() const { return n_ * sizeof(T); }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace ws
