// A std::vector handed to numpy without a copy (the array owns it), for the units of _tbhost.
#pragma once
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <vector>

template <class T>
static pybind11::array_t<T> to_numpy(std::vector<T>&& v) {
  namespace py = pybind11;
  auto* heap = new std::vector<T>(std::move(v));
  py::capsule owner(heap, [](void* p) { delete reinterpret_cast<std::vector<T>*>(p); });
  return py::array_t<T>({(py::ssize_t)heap->size()}, {(py::ssize_t)sizeof(T)}, heap->data(), owner);
}
