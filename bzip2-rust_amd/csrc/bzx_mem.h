// bzx_mem.h -- who owns device and page-locked memory on the host side (internal, not installed).
//
// Mem is a move-only owner of ONE allocation: DevMem of hipMalloc memory, PinMem of hipHostMalloc memory.  It records no
// device and sets none: it frees with whatever device is current, so an object that lives on another device sets it
// first, and an object with work in flight waits for its streams first and then resets (or deletes) its members -- the
// order stays written out in bzx_ctx_destroy, bzx_dstream_end, ChunkLane::free and mstream_free ("Who owns
// memory").  Growth policies (floors, pads, 1.5x) are the argument of reserve at the call site, and so is the error text.
//
// Carver is the layout of a workspace that holds several tables: the layout is written once, as a function over a
// Carver, and carved() runs it twice -- over a null base for the size, over the real base for the pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

template <bool PINNED, typename T = uint8_t> class Mem {
    void *p_ = nullptr;
    size_t bytes_ = 0;

public:
    Mem() = default;
    Mem(const Mem &) = delete;
    Mem &operator=(const Mem &) = delete;
    Mem(Mem &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
    ~Mem() { reset(); }
    // Grow-only: nothing happens while `bytes` fit; else the old allocation goes and one of `bytes` comes (its contents
    // are not kept).  false: the allocation failed, and the object holds nothing.  flags: hipHostMalloc's (PinMem).
    bool reserve(size_t bytes, unsigned flags = 0)
    {
        if (bytes <= bytes_) return true;
        reset();
        const hipError_t e = PINNED ? hipHostMalloc(&p_, bytes, flags) : hipMalloc(&p_, bytes);
        if (e != hipSuccess) {
            p_ = nullptr;
            return false;
        }
        bytes_ = bytes;
        return true;
    }
    void reset()
    {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        bytes_ = 0;
    }
    template <typename U = T> U *get() const { return static_cast<U *>(p_); }
    // A member of a fixed element type reads as the pointer it owns -- but not as a kernel argument: a launch takes its
    // arguments by value, and an owner is not copied.  Pass get() there.
    operator T *() const { return get(); }
    size_t bytes() const { return bytes_; }
};
template <typename T = uint8_t> using DevMem = Mem<false, T>;
template <typename T = uint8_t> using PinMem = Mem<true, T>;

class Carver {
    uint8_t *base_;
    size_t align_, at_ = 0;

public:
    Carver(void *base, size_t align) : base_(static_cast<uint8_t *>(base)), align_(align) {}
    // count elements of T, padded to the alignment (a power of two; the base is aligned at least as much)
    template <typename T> T *take(size_t count)
    {
        uint8_t *p = base_ ? base_ + at_ : nullptr;
        at_ += (count * sizeof(T) + align_ - 1) & ~(align_ - 1);
        return reinterpret_cast<T *>(p);
    }
    size_t bytes() const { return at_; }
};

// The workspace `layout` describes, in `mem`: sized by a first run of the layout, grown if it has to be, carved by a
// second.  false: the allocation failed.
template <bool PINNED, typename T, typename F> static inline bool carved(Mem<PINNED, T> &mem, size_t align, F &&layout)
{
    Carver size(nullptr, align);
    layout(size);
    if (!mem.reserve(size.bytes())) return false;
    Carver c(mem.template get<void>(), align);
    layout(c);
    return true;
}
