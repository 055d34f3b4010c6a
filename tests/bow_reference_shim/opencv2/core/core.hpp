// Stand-in for <opencv2/core/core.hpp> when tests/golden/make_bow_reference.py compiles the reference's DBoW2 (TemplatedVocabulary.h,
// FORB.cpp, BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp) for tests/bow_reference_driver.cpp: the cv::Mat members FORB uses, on
// a byte vector with value semantics, and a cv::FileStorage / cv::FileNode that only has to compile (the driver loads text files).
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
 public:
    int rows = 0, cols = 0;
    Mat() {}
    void create(int r, int c, int type) {
        rows = r; cols = c; elem_ = type == CV_32F ? 4 : 1;
        buf_.assign((size_t)r * (size_t)c * elem_, 0);
    }
    static Mat zeros(int r, int c, int type) { Mat m; m.create(r, c, type); return m; }
    Mat clone() const { return *this; }
    void release() { rows = cols = 0; buf_.clear(); }
    bool empty() const { return buf_.empty(); }
    template <class T> T *ptr(int r = 0) { return reinterpret_cast<T *>(buf_.data() + (size_t)r * (size_t)cols * elem_); }
    template <class T> const T *ptr(int r = 0) const { return reinterpret_cast<const T *>(buf_.data() + (size_t)r * (size_t)cols * elem_); }

 private:
    size_t elem_ = 1;
    std::vector<unsigned char> buf_;
};

class FileNode {
 public:
    FileNode operator[](const char *) const { return FileNode(); }
    FileNode operator[](const std::string &) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator double() const { return 0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
 public:
    enum { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const char *, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const std::string &) const { return FileNode(); }
    template <class T> FileStorage &operator<<(const T &) { return *this; }
};

}  // namespace cv
