// Layout of one device buffer, decided on the host: a staged prefix of host arrays (one upload) and, behind it, regions only the device
// touches. The byte counts and every pointer come from the list of what was appended, so a size and a layout cannot disagree.
// Host only, no HIP header: the buffer itself comes from whoever uses the image (a plan's own block, a workspace, the staging ring).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// A typed place in the buffer: byte offset and element count.
template <class T>
struct image_slot {
  size_t offset = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
  T*     at(void* base) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + offset); }
  T*     at(const void* base) const { return at(const_cast<void*>(base)); } // (the staging ring hands out const pointers)
};

class device_image {
public:
  // Appends the array to the staged part at a 16-byte boundary. The elements are read by copy_staged(): `src` outlives the image.
  // After the first reserve() the staged part is closed: the put is refused, ok() turns false and nothing accepts the image.
  template <class T>
  image_slot<T> put(const T* src, size_t count)
  {
    if (closed_) {
      ok_ = false;
      return {};
    }
    const image_slot<T> s = {append(count * sizeof(T), 16), count};
    if (count)
      parts_.push_back({src, s.offset, s.bytes()});
    staged_ = total_;
    return s;
  }
  template <class T>
  image_slot<T> put(const std::vector<T>& v)
  {
    return put(v.data(), v.size());
  }
  template <class T>
  image_slot<T> put(std::vector<T>&&) = delete; // (a temporary would be gone before copy_staged)

  // Appends a region behind the staged part that is not uploaded; align: a power of two.
  template <class T>
  image_slot<T> reserve(size_t count, size_t align = 16)
  {
    closed_ = true;
    return {append(count * sizeof(T), align), count};
  }

  bool   ok() const { return ok_; }
  size_t staged_bytes() const { return staged_; } // the prefix that is uploaded: every put array, gaps included
  size_t total_bytes() const { return total_; }   // the whole buffer

  // Writes the staged part to dst[0 .. staged_bytes()): the one host copy between the arrays and the upload. Gaps are zeroed.
  void copy_staged(void* dst) const
  {
    if (!staged_)
      return;
    uint8_t* d   = static_cast<uint8_t*>(dst);
    size_t   end = 0;
    for (const part& p : parts_) {
      std::memset(d + end, 0, p.offset - end);
      std::memcpy(d + p.offset, p.src, p.bytes);
      end = p.offset + p.bytes;
    }
    std::memset(d + end, 0, staged_ - end);
  }
  std::vector<uint8_t> staged() const
  {
    std::vector<uint8_t> h(staged_);
    copy_staged(h.data());
    return h;
  }

  template <class T>
  static T* at(void* base, const image_slot<T>& s)
  {
    return s.at(base);
  }

private:
  struct part {
    const void* src;
    size_t      offset, bytes;
  };
  size_t append(size_t bytes, size_t align)
  {
    const size_t off = (total_ + align - 1) & ~(align - 1);
    total_           = off + bytes;
    return off;
  }
  std::vector<part> parts_;
  size_t            staged_ = 0, total_ = 0;
  bool              closed_ = false, ok_ = true;
};
