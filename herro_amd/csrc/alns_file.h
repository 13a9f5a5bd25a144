// alns_file.h — the file herro_pairs_write_alns (frontend_api.hip) streams its text to (ingest.cpp): plain, or one zstd frame at level 0 through the
// system's libzstd.so.1 as AlnMode::Write produces it (overlaps.rs:270-282).  Everything goes to path + ".tmp"; commit() renames it to path, and a
// file that is not committed is removed, so a failing call leaves nothing behind.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

struct AlnsFile {
  AlnsFile() = default;
  AlnsFile(const AlnsFile&) = delete;
  AlnsFile& operator=(const AlnsFile&) = delete;
  ~AlnsFile();
  // false with `why`; unsupported: zstd was asked for and libzstd.so.1 is not available
  bool open(const char* path, bool zstd, std::string& why, bool& unsupported);
  bool write(const char* p, size_t n, std::string& why);
  bool commit(std::string& why);
  double zstd_seconds = 0;   // spent inside the compressor
  uint64_t file_bytes = 0;   // written to the file

 private:
  bool flush_out(size_t n, std::string& why);
  std::string path_, tmp_;
  FILE* f_ = nullptr;
  void* cs_ = nullptr;       // ZSTD_CStream
  std::vector<char> ob_;
};
