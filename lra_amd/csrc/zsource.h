// lra_amd/csrc/zsource.h -- where the readers' compressed bytes come from: the one BGZF / gzip layer under the read files (input.hip, input_device.hip), BAM
// (the same two) and the genome FASTA (genome.hip).  The rules of a BGZF member, the texts of a compression fault and the file-read loop live here once,
// so the host and device forms of every reader say the same thing about the same file.  A source's error text lacks the file's name: its owner puts
// "<path>: " in front.
#pragma once
#include "common.h"
#include "bam_kernels.h"
#include "bgzf.h"
#include "byte_tiles.h"
#include <string>
#include <vector>

const char* lra_bgzf_reason(int status);          // a bgzf.h status in words
const char* lra_gz_reason(int status);            // a status of lra_gz_step in words
int lra_bgzf_inflate_one(const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t isize);   // a member, host side: inflate, ISIZE, CRC-32 (a bgzf.h status)

// Up to `want` bytes of fd into dst: *got of them, less than `want` only at the end of the file.  false: read() failed (*got bytes stand)
bool lra_read_all(int fd, void* dst, uint64_t want, uint64_t* got);

// The whole members at the front of h[0, len): in_off / out_off = nb + 1 offsets each, compressed from 0, decoded from `carry`; p = the byte behind the
// last whole member; block_err = why the walk stopped in front of h[p], if that is a fault ("not a BGZF block", "the file ends inside it", "a bad
// ISIZE").  starved: no whole member, no fault and more of the file to read -- the caller reads on, twice as much.
struct lra_bgzf_members {
  std::vector<uint64_t> in_off, out_off;
  uint64_t p = 0;
  const char* block_err = nullptr;
  bool starved = false;
};
lra_bgzf_members lra_bgzf_walk(const uint8_t* h, uint64_t len, bool file_eof, uint64_t carry);

// One step of a BGZF file on the device: whole members of the compressed bytes read so far (a member the step cut stays on the host for the next one),
// inflated a wave per member behind the carried tail of the last step's data -- what its reader did not consume, carried device to device.
typedef void (*lra_inflate_launch)(hipStream_t st, int n, const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off, uint8_t* out, int32_t* status);
struct lra_bgzf_step {
  PinBuf<char> h_comp; uint64_t comp_len = 0, consumed = 0;   // compressed bytes read ahead; those in front of `consumed` are done with
  uint64_t file_off = 0;                           // file offset of h_comp[0]
  bool file_eof = false;                           // every byte of the file is in h_comp
  DevBuf<uint8_t> d_comp, d_dec[2]; DevBuf<uint64_t> d_boff; DevBuf<int32_t> d_bstat;
  int cur = 0; uint64_t dec_len = 0, dec_used = 0; // the last committed step's data is d_dec[cur][0, dec_len); [dec_used, dec_len) is the carry
  // what fill() found
  const uint8_t* data = nullptr; uint64_t dlen = 0;   // the step's data: the carry, then the members in front of the first fault; zeros up to padded_tiles(dlen)
  uint64_t stop = 0;                               // the compressed bytes the step's members take
  std::vector<uint64_t> in_off, out_off;           // the step's member table (lra_bgzf_members'): compressed offsets from file_off, decoded offsets in data
  bool at_end = false;                             // no byte of the file's data is behind this step: the end of the file, or a fault (err)
  std::string err;                                 // the BGZF fault text (zsource.hip: offset and reason): a member's status wins over the walk's stop
  size_t nomem_pinned = 0;                         // fill() returned LRA_ERR_NOMEM: the page-locked bytes it asked for (0: a device allocation failed)
  void reset() {                                   // a new file: no bytes read, no carry, nothing found (the buffers stay)
    comp_len = consumed = file_off = dec_len = dec_used = dlen = stop = 0; cur = 0; file_eof = at_end = false; data = nullptr; err.clear();
  }
  // Reads `*want` more bytes (unless the file is over), walks, uploads, carries, inflates (launch: lra_bgzf_launch_inflate or _lut) and checks the
  // statuses; reads on, doubling *want, while no whole member is there.  The carry and `cur` stay: a caller that finds no whole record in the data
  // calls again with a larger *want.  h2d / inflate: the timing names (string literals: the context keeps the pointers).  Returns LRA_OK, LRA_ERR_HIP
  // (the context's error is set), or -- bare, the caller words them -- LRA_ERR_NOMEM (an allocation failed: nomem_pinned) or LRA_ERR_INVALID (read() failed).
  int fill(lra_ctx* ctx, int fd, uint64_t* want, lra_inflate_launch launch, const char* h2d, const char* inflate);
  void commit(uint64_t used);                      // the caller took data[0, used): the rest is the next step's carry, the members are consumed
  void release();
};

// The next whole BGZF member from a read-ahead buffer, on the host.  (refill() moves the unconsumed bytes, less than one member or one read, to the
// buffer's front before every read.)
struct lra_bgzf_source {
  int fd = -1;
  std::vector<uint8_t> comp; size_t pos = 0;       // compressed bytes read ahead: comp[pos..] are not consumed
  uint64_t file_off = 0;                           // file offset of comp[0]
  bool file_eof = false, read_failed = false;      // (a failed read ends the file)
  uint32_t member_len = 0;                         // of the member peek() found
  std::string err;                                 // the BGZF fault text (zsource.hip: offset and reason)
  bool refill(size_t want);                        // reads on; false: nothing came
  bool at_end() const { return file_eof && pos == comp.size(); }   // every byte of the file is consumed
  void clear() { std::vector<uint8_t>().swap(comp); pos = 0; }     // frees the read-ahead
  bool peek(uint32_t* isize);                      // a whole member stands at comp[pos], its ISIZE; false: the end of the file, or a fault (err)
  bool take(uint8_t* out);                         // that member inflated into out[0, isize) and consumed; false: a fault (err)
};

// The first `hdr` bytes of the BGZF file at `path`, uncompressed -- a BAM file's header, as lra_hts_sniff sized it -- member by member on the host.
// false: *why says what is wrong with the file, without its name.
bool lra_bam_read_header(const std::string& path, uint64_t hdr, std::vector<uint8_t>& out, std::string& why);

// gzip that is not BGZF: one serial bit stream over the whole compressed file as one array (lra_gz_stream), inflated a step at a time on the host
struct lra_gzip_source {
  std::vector<uint8_t> comp;
  lra_gz_stream gz;
  bool done = false;                               // no byte of the file's data is behind the last step: the end of the file, or a fault (err)
  std::string err;                                 // the gzip fault text (zsource.hip: offset and reason); dst[0, *got) is the data in front of it
  bool load(int fd);                               // false: read() failed
  void step(uint8_t* dst, uint64_t cap, uint64_t* got);
};
